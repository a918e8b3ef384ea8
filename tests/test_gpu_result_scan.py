"""GPU check of k_result_scan, the one-block scan every result pass (diff, checkout, blame, encode,
lines, find) turns its per-index counts into offsets with, at a list long enough that its threads
own slices of several results.

With n = 2,051 indexes and 1,024 threads a slice holds per = 3 results: threads 0..682 own three,
thread 683 owns two (the partial last slice), threads 684..1,023 own none.  Indexes without a result
(0, the last one, 1,024 and 1,025 inside the slice of the ordinary 1,023, and two that would
otherwise count 3) must count as 0 wherever they sit.  Every per-index result is compared exactly
with the Python references, applied to the engine's own export and text; a second, 5-index call on
the same engine then reuses the buffers of the first.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from blame_ref import ref_blame  # noqa: E402
from checkout_ref import ref_checkout  # noqa: E402
from diff_ref import ref_diff  # noqa: E402
from encode_ref import UTF8, UTF16, ref_encode  # noqa: E402
from find_ref import ref_find  # noqa: E402
from lines_ref import EOL_LF, ref_lines  # noqa: E402

N = 2051
NO_RESULT = 0xFFFFFFFF
BAD = (0, 7, 1024, 1025, 1027, N - 1)  # no content; since / version above the document's
SHORT = [2049, 3, 1027, 6, 1026]       # the second call's list (one index without a result)
NEEDLE = "ab"
ENCS = {"utf8": UTF8, "utf16": UTF16}


def text_of(d: int) -> np.ndarray:
    """d mod 4 characters: a rotation of "ab\\n" cut short, so the newline and the needle move"""
    r = (d // 4) % 3
    s = ("ab\n" * 2)[r:r + 3][:d % 4]
    return np.array([ord(c) for c in s], np.uint32)


@pytest.fixture(scope="module")
def corpus():
    """the engine, every document's export and, where content is set, its text (read once, shared)"""
    e = crdt_amd.Engine(N, 32)
    docs = list(range(N))
    texts = [text_of(d) for d in docs]
    ag = e.agent_intern(docs, ["xa"] * N)
    assert (e.apply_local([(d, [(int(ag[d]), [(0, 0, len(t))])]) for d, t in enumerate(texts) if len(t)]) == 0).all()
    with_content = [d for d in docs if d not in BAD]
    e.set_content(with_content, list(range(len(with_content))), [texts[d] for d in with_content])
    assert (e.versions() == np.arange(N) % 4).all()
    exports = [e.export(d) for d in docs]
    own = {d: e.text(d) for d in with_content}
    assert all(np.array_equal(own[d], texts[d]) for d in with_content)
    yield e, exports, own
    e.close()


def both_lists(check):
    """`check(docs)` over all N indexes, then over the short list on the same engine"""
    check(list(range(N)))
    check(SHORT)


def test_diff_from_version_zero(corpus):
    e, exports, _ = corpus
    ver = e.versions()

    def check(docs):
        since = [int(ver[d]) + 1 if d in BAD else 0 for d in docs]
        e.diff_async(docs, since)
        npat, nins = e.diff_counts()
        want_p = want_i = 0
        for i, d in enumerate(docs):
            if d in BAD:
                assert int(npat[i]) == NO_RESULT and int(nins[i]) == NO_RESULT, (i, d)
                continue
            wp, wi = ref_diff(exports[d], 0)
            pat, io, _ = e.diff_read(i, (npat, nins), text=False)
            assert pat.shape == wp.shape and np.array_equal(pat, wp), (i, d, pat, wp)
            assert np.array_equal(io, wi), (i, d)
            want_p += wp.shape[0]
            want_i += wi.shape[0]
        good = npat != NO_RESULT
        assert int(npat[good].sum()) == want_p and int(nins[good].sum()) == want_i
        assert want_p > 0 and want_i > 0

    both_lists(check)


def test_checkout_at_the_current_version(corpus):
    e, exports, _ = corpus
    ver = e.versions()

    def check(docs):
        at = [int(ver[d]) + (1 if d in BAD else 0) for d in docs]
        res = e.checkout(docs, at, strict=False)
        lens = e.checkout_lens()
        want_n = 0
        for i, d in enumerate(docs):
            if d in BAD:
                assert res[i] is None and int(lens[i]) == NO_RESULT, (i, d)
                continue
            want = ref_checkout(exports[d], at[i])
            assert res[i][0].shape == want.shape and np.array_equal(res[i][0], want), (i, d, res[i][0], want)
            want_n += want.shape[0]
        assert int(lens[lens != NO_RESULT].sum()) == want_n > 0

    both_lists(check)


def test_blame_by_id(corpus):
    e, exports, _ = corpus

    def check(docs):
        res = e.blame(docs, "id")  # (every index has a result: no document is poisoned)
        counts = e.blame_counts()
        want_n = 0
        for i, d in enumerate(docs):
            want = ref_blame(exports[d], "id")
            assert res[i].shape == want.shape and np.array_equal(res[i], want), (i, d, res[i], want)
            want_n += want.shape[0]
        assert int(counts.sum()) == want_n > 0

    both_lists(check)


@pytest.mark.parametrize("encname", ["utf8", "utf16"])
def test_encode_lines_and_find(corpus, encname):
    e, _, own = corpus
    enc = ENCS[encname]
    needle = np.array([ord(c) for c in NEEDLE], np.uint32)

    def check(docs):
        res = e.encode(docs, encname, strict=False)
        units, chars = e.encode_lens()
        lines = e.lines("lf", strict=False)
        n_lines = e.line_counts()
        found = e.find(NEEDLE, strict=False)
        n_found = e.find_counts()
        want_u = want_l = want_f = 0
        for i, d in enumerate(docs):
            if d in BAD:
                assert res[i] is None and lines[i] is None and found[i] is None, (i, d)
                assert int(units[i]) == int(n_lines[i]) == int(n_found[i]) == NO_RESULT, (i, d)
                continue
            wu, start = ref_encode(own[d], enc)
            got = np.frombuffer(res[i], np.uint8) if enc == UTF8 else res[i]
            assert got.dtype == wu.dtype and got.shape == wu.shape and np.array_equal(got, wu), (i, d, got, wu)
            assert int(chars[i]) == len(own[d])
            wl = ref_lines(own[d], start, EOL_LF)
            assert lines[i].shape == wl.shape and np.array_equal(lines[i], wl), (i, d, lines[i], wl)
            wf = ref_find(own[d], start, needle)
            assert found[i].shape == wf.shape and np.array_equal(found[i], wf), (i, d, found[i], wf)
            want_u += len(wu)
            want_l += len(wl)
            want_f += len(wf)
        assert int(units[units != NO_RESULT].sum()) == want_u > 0
        assert int(n_lines[n_lines != NO_RESULT].sum()) == want_l > 0
        assert int(n_found[n_found != NO_RESULT].sum()) == want_f > 0

    both_lists(check)
