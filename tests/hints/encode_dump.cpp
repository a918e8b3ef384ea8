// TEST INFRASTRUCTURE: prints the record stream the host encoder makes of remote wire batches
// (host_plan.h WireView::parse + encode_remote), for tests/test_delete_hints.py.
//
//   encode_dump WIRE                 one batch
//   encode_dump WIRE --append WIRE2  a second batch staged onto the same stream (same agent table)
//   encode_dump -q ...               exit 3 for a malformed wire without the message on stderr
//                                    (tests/test_wire_malformed.py: anything on stderr is a sanitizer's)
//
// Exit status: 0 printed, 2 usage or unreadable file, 3 malformed wire (WireView::parse refused it).
// One line per record: "<batch> <w0> <w1> <w2> <w3>" (batch 0 or 1, words in hex).  A stand-alone
// host program: built with -fsanitize=address,undefined by the test, nothing else linked.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_plan.h"

using namespace crdt;

// a wire file in 4-byte aligned storage (WireView keeps u32 pointers into it) of exactly its
// length (operator new[] aligns to 16): a read one byte past the wire is a sanitizer report
static bool read_file(const char* path, std::unique_ptr<uint8_t[]>& bytes, size_t& len) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::vector<uint8_t> b;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
  std::fclose(f);
  len = b.size();
  bytes.reset(new uint8_t[len ? len : 1]);
  if (len) std::memcpy(bytes.get(), b.data(), len);
  return true;
}

int main(int argc, char** argv) {
  bool quiet = argc > 1 && std::string(argv[1]) == "-q";
  if (quiet) { argc--; argv++; }
  if (!(argc == 2 || (argc == 4 && std::string(argv[2]) == "--append"))) {
    std::fprintf(stderr, "usage: encode_dump [-q] WIRE [--append WIRE2]\n");
    return 2;
  }
  std::vector<Rec> out;
  StreamNeeds nd;
  AgentTable at;
  size_t first_n = 0;
  for (int b = 0; b < (argc == 4 ? 2 : 1); b++) {
    std::unique_ptr<uint8_t[]> bytes;
    size_t len = 0;
    if (!read_file(argv[b == 0 ? 1 : 3], bytes, len)) {
      std::fprintf(stderr, "cannot read %s\n", argv[b == 0 ? 1 : 3]);
      return 2;
    }
    WireView wv;
    if (!wv.parse(bytes.get(), len)) {
      if (!quiet) std::fprintf(stderr, "malformed wire %s\n", argv[b == 0 ? 1 : 3]);
      return 3;
    }
    encode_remote(out, nd, at, wv);  // (wv's pointers into `bytes` are not used after this call)
    if (b == 0) first_n = out.size();
  }
  for (size_t i = 0; i < out.size(); i++)
    std::printf("%d %08x %08x %08x %08x\n", i < first_n ? 0 : 1, out[i].w0, out[i].w1, out[i].w2, out[i].w3);
  return 0;
}
