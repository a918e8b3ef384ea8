// TEST INFRASTRUCTURE: prints the record stream the host encoder makes of remote wire batches
// (host_plan.h WireView::parse + encode_remote), for tests/test_delete_hints.py.
//
//   encode_dump WIRE                 one batch
//   encode_dump WIRE --append WIRE2  a second batch staged onto the same stream (same agent table)
//
// One line per record: "<batch> <w0> <w1> <w2> <w3>" (batch 0 or 1, words in hex).  A stand-alone
// host program: built with -fsanitize=address,undefined by the test, nothing else linked.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_plan.h"

using namespace crdt;

// a wire file in 4-byte aligned storage (WireView keeps u32 pointers into it)
static bool read_file(const char* path, std::vector<u32>& words, size_t& len) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::vector<uint8_t> b;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
  std::fclose(f);
  len = b.size();
  words.assign((len + 3) / 4 + 1, 0u);
  if (len) std::memcpy(words.data(), b.data(), len);
  return true;
}

int main(int argc, char** argv) {
  if (!(argc == 2 || (argc == 4 && std::string(argv[2]) == "--append"))) {
    std::fprintf(stderr, "usage: %s WIRE [--append WIRE2]\n", argv[0]);
    return 2;
  }
  std::vector<Rec> out;
  StreamNeeds nd;
  AgentTable at;
  size_t first_n = 0;
  for (int b = 0; b < (argc == 4 ? 2 : 1); b++) {
    std::vector<u32> words;
    size_t len = 0;
    if (!read_file(argv[b == 0 ? 1 : 3], words, len)) {
      std::fprintf(stderr, "cannot read %s\n", argv[b == 0 ? 1 : 3]);
      return 2;
    }
    WireView wv;
    if (!wv.parse((const uint8_t*)words.data(), len)) {
      std::fprintf(stderr, "malformed wire %s\n", argv[b == 0 ? 1 : 3]);
      return 3;
    }
    encode_remote(out, nd, at, wv);  // (wv's pointers into `words` are not used after this call)
    if (b == 0) first_n = out.size();
  }
  for (size_t i = 0; i < out.size(); i++)
    std::printf("%d %08x %08x %08x %08x\n", i < first_n ? 0 : 1, out[i].w0, out[i].w1, out[i].w2, out[i].w3);
  return 0;
}
