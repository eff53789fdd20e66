"""GPU (-m gpu): the wave-wide scans of csrc/wave_scan.hpp (DPP row steps + carries between the rows through v_readlane) through the probe
kamd_debug_wave_scan -- one wavefront per case of 64 lanes, all lanes active.  Every result must equal the numpy restatement below exactly: inclusive
sum, inclusive sum inside segments, inclusive OR of a 64-bit value (two words) inside segments, and the wave total read from lane 63."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_EDGES = (0, 15, 16, 31, 32, 47, 48, 63)                 # first and last lane of every DPP row
SEGMENT_STARTS = (0, 1, 15, 16, 17, 31, 32, 47, 48, 63)
OR_BITS = (0, 31, 32, 63)


def start_lanes(first_lanes):
    """per lane the first lane of its segment, from the lanes at which a segment begins (lane 0 always begins one: 0 = it began before this wavefront)"""
    s = np.zeros(64, np.uint32)
    cur = 0
    for lane in range(64):
        if lane in first_lanes:
            cur = lane
        s[lane] = cur
    return s


def restate(x, start, v64):
    """the three scans lane by lane"""
    tot = np.zeros(64, np.uint32)
    seg = np.zeros(64, np.uint32)
    orv = np.zeros(64, np.uint64)
    for lane in range(64):
        tot[lane] = np.uint32(int(x[:lane + 1].astype(np.uint64).sum()) & 0xFFFFFFFF)
        a = int(start[lane])
        seg[lane] = np.uint32(int(x[a:lane + 1].astype(np.uint64).sum()) & 0xFFFFFFFF)
        orv[lane] = np.bitwise_or.reduce(v64[a:lane + 1])
    return tot, seg, orv


def cases():
    rng = np.random.default_rng(20250)
    zeros, ones = np.zeros(64, np.uint32), np.ones(64, np.uint32)
    none = start_lanes(())
    bits = np.array([1 << b for b in OR_BITS], np.uint64)
    out = []

    def add(x, start, v64):
        out.append((np.asarray(x, np.uint32), np.asarray(start, np.uint32), np.asarray(v64, np.uint64)))

    all_bits = np.full(64, np.bitwise_or.reduce(bits), np.uint64)
    # all-zero and all-ones inputs, with no segment start and with one at every listed lane
    for x, v in ((zeros, np.zeros(64, np.uint64)), (ones, all_bits), (np.full(64, 0xFFFFFFFF, np.uint32), np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64))):
        add(x, none, v)
        for s in SEGMENT_STARTS:
            add(x, start_lanes((s,)), v)
        add(x, start_lanes(SEGMENT_STARTS), v)
        add(x, np.arange(64, dtype=np.uint32), v)            # every lane a segment of its own
    # a single 1 / a single OR bit at each row edge, under every segment start (and none)
    for lane in ROW_EDGES:
        x = zeros.copy()
        x[lane] = 1
        for b in OR_BITS:
            v = np.zeros(64, np.uint64)
            v[lane] = np.uint64(1 << b)
            add(x, none, v)
            for s in SEGMENT_STARTS:
                add(x, start_lanes((s,)), v)
            add(x, start_lanes(SEGMENT_STARTS), v)
    # 256 seeded random cases: counts as the kernel scans them, random 64-bit masks, random segment starts (sparse and dense)
    for i in range(256):
        x = rng.integers(0, 1 << (1 + i % 24), 64, dtype=np.uint64).astype(np.uint32)
        v = rng.integers(0, 1 << 63, 64, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 64, dtype=np.uint64)
        v &= np.where(rng.random(64) < 0.5, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)) if i % 2 else np.uint64(0xFFFFFFFFFFFFFFFF)
        firsts = tuple(int(l) for l in np.nonzero(rng.random(64) < (0.02, 0.1, 0.3, 0.7)[i % 4])[0])
        add(x, start_lanes(firsts), v)
    return out


def test_wave_scans_equal_the_numpy_restatement():
    lib = C.CDLL(os.path.join(ROOT, "kiwi_amd", "libkiwi_hip.so"))
    lib.kamd_debug_wave_scan.restype = C.c_int
    lib.kamd_debug_wave_scan.argtypes = [C.c_void_p] * 9 + [C.c_uint32]
    cs = cases()
    n = len(cs)
    x = np.ascontiguousarray(np.concatenate([c[0] for c in cs]))
    start = np.ascontiguousarray(np.concatenate([c[1] for c in cs]))
    v64 = np.concatenate([c[2] for c in cs])
    lo = np.ascontiguousarray((v64 & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    hi = np.ascontiguousarray((v64 >> np.uint64(32)).astype(np.uint32))
    got = [np.full(64 * n, 0xCDCDCDCD, np.uint32) for _ in range(4)]
    last = np.full(n, 0xCDCDCDCD, np.uint32)
    rc = lib.kamd_debug_wave_scan(x.ctypes.data, start.ctypes.data, lo.ctypes.data, hi.ctypes.data, got[0].ctypes.data, got[1].ctypes.data, got[2].ctypes.data,
                                  got[3].ctypes.data, last.ctypes.data, n)
    assert rc == 0
    for i, (cx, cstart, cv) in enumerate(cs):
        tot, seg, orv = restate(cx, cstart, cv)
        sl = slice(64 * i, 64 * i + 64)
        assert (got[0][sl] == tot).all(), ("sum", i, cx.tolist())
        assert (got[1][sl] == seg).all(), ("segmented sum", i, cx.tolist(), cstart.tolist())
        got_or = got[2][sl].astype(np.uint64) | (got[3][sl].astype(np.uint64) << np.uint64(32))
        assert (got_or == orv).all(), ("segmented or", i, [hex(int(t)) for t in cv], cstart.tolist())
        assert last[i] == tot[63], ("wave total", i)
