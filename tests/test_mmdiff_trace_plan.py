"""CPU checks of how a traced mmdiff run is cut into launches (mmg_selftest_diff_trace_plan: the functions mmg_diff_trace_open and
the traced phases call, no device): every launch's rows fit the buffer, the launches tile the phase, and their rows are the recorded
iterations in order -- for buffers smaller than a full launch's rows too, which is what a default-size run has.  And the refusal of
thinning intervals outside 1 .. 2^30."""
import ctypes as C

import pytest

from mmseq_amd import _lib

CHUNK = 512


def plan(P, F, every_min, max_rows, tt, left, every):
    lib = _lib.load()
    out = [C.c_uint32() for _ in range(4)]
    _lib.check(lib.mmg_selftest_diff_trace_plan(P, F, every_min, max_rows, tt, left, every, *(C.byref(v) for v in out)))
    return tuple(v.value for v in out)          # cap, first_row, rows, n


def launches(P, F, every_min, max_rows, tt0, iters, every):
    out, j = [], 0
    while j < iters:
        cap, first, rows, n = plan(P, F, every_min, max_rows, tt0 + j, iters - j, every)
        assert 1 <= n <= min(CHUNK, iters - j) and rows <= cap
        assert [first + r for r in range(rows)] == [t // every for t in range(tt0 + j, tt0 + j + n) if t % every == 0]
        out.append((first, rows, n))
        j += n
    assert j == iters
    return out


@pytest.mark.parametrize("every", [1, 3, 5, 7, 8, 16, 511, 512, 513, 2000])
@pytest.mark.parametrize("max_rows", [0, 1, 2, 5, 29])
@pytest.mark.parametrize("tt0,iters", [(0, 1100), (0, 1024), (600, 700), (13, 1), (1024, 2048)])
def test_launches_tile_the_phase_and_fit_the_buffer(every, max_rows, tt0, iters):
    ls = launches(14, 130, every, max_rows, tt0, iters, every)
    want_rows = len([t for t in range(tt0, tt0 + iters) if t % every == 0])
    assert sum(r for _, r, _ in ls) == want_rows
    if max_rows == 0:                           # the buffer holds a full launch: the launches of the untraced loop
        assert [n for _, _, n in ls] == [min(CHUNK, iters - j) for j in range(0, iters, CHUNK)]
    elif every * (max_rows + 1) <= CHUNK:       # shortened: a launch ends before the row after the buffer's last
        assert max(n for _, _, n in ls) < every * (max_rows + 1)


def test_the_coarser_phase_uses_the_buffer_of_the_denser_one():
    # every = 7 in burn-in, 5 in sampling: 103 rows; a burn-in launch needs 74
    assert plan(14, 130, 5, 0, 0, 1100, 7) == (103, 0, 74, 512)
    assert plan(14, 130, 5, 0, 512, 588, 7) == (103, 74, 73, 512)
    assert plan(14, 130, 5, 0, 512, 88, 5) == (103, 103, 17, 88)


def test_default_size_run_is_cut_by_the_64_mib_limit():
    """20 000 features, 14 traced parameters: a row is 2 240 000 bytes and 64 MiB hold 29 of them, fewer than the 64 and 32 rows of a
    full launch at every = 8 and 16.  At 200 000 features 2 rows; at 10 million one row, not none."""
    assert (64 << 20) // (14 * 20000 * 8) == 29
    assert plan(14, 20000, 8, 0, 0, 8192, 8) == (29, 0, 29, 232)
    assert plan(14, 20000, 8, 0, 232, 8192 - 232, 8) == (29, 29, 29, 232)
    assert plan(14, 20000, 8, 0, 0, 16384, 16) == (29, 0, 29, 464)
    assert plan(14, 200000, 8, 0, 0, 8192, 8) == (2, 0, 2, 16)
    assert plan(14, 10_000_000, 8, 0, 0, 8192, 8) == (1, 0, 1, 8)
    assert len(launches(14, 20000, 8, 0, 0, 8192, 8)) == 36          # 35 of 232 iterations and one of 72


def test_largest_interval():
    big = 1 << 30
    assert plan(14, 130, big, 0, 0, 1024, big) == (1, 0, 1, 512)
    assert plan(14, 130, big, 0, 512, 512, big) == (1, 1, 0, 512)


@pytest.mark.parametrize("eb,es", [(0, 1), (1, 0), ((1 << 30) + 1, 1), (1, 1 << 31), (0x80000001, 1), (1, 0xFFFFFFFF), (0xFFFFFE01, 0xFFFFFE01)])
def test_intervals_outside_1_to_2_pow_30_are_refused(eb, es):
    """Checked before anything else, so no handle is needed: beyond 2^30 the row arithmetic of the kernel would leave int."""
    lib = _lib.load()
    assert lib.mmg_diff_trace_open(None, eb, es, None, None) == 1
    assert b"at least 1 and at most 1073741824" in lib.mmg_last_error()
    assert lib.mmg_diff_trace_open(None, 1 << 30, 1, None, None) == 1 and b"NULL argument" in lib.mmg_last_error()
    for bad in ((14, 130, 0, 0, 0, 1, 1), (14, 130, 1, 0, 0, 1, (1 << 30) + 1), (14, 130, 1, 0, 0, 0, 1)):
        out = [C.c_uint32() for _ in range(4)]
        assert lib.mmg_selftest_diff_trace_plan(*bad, *(C.byref(v) for v in out)) == 1
