"""Shared by tests/test_pos_step_head_cpu.py (lane emulator) and tests/test_gpu_pos_step_head.py (device): the inputs of the parity cases for the head of a
position step -- the records of a step are its first loads, the table entries and predecessor ranges of the following steps are fetched behind them, and the
lane groups form the addresses of their chunk's tables from 32-bit offsets.  The comparison itself is tests/pos_rounds_cases.py's `check`: the
position-step kernel == the CPU oracle analysis for analysis, and == the general search kernel (KAMD_POS_PATH=0) of the same library."""
from corpora import EDGE_TEXTS
from pos_rounds_cases import mixed_texts

# One, two and three text units (open syllables: a syllable with a coda is two units), i.e. lattices of one to three end positions: the fetch of the table entry
# two steps ahead and of the next step's predecessor ranges and item multipliers reaches the end of the position table in the very first step.
ONE_POSITION = ["가", "이", "a", "1", "."]
TWO_POSITIONS = ["가나", "하다", "이가", "ab", "가."]
THREE_POSITIONS = ["가나다", "하였다", "사과가", "가 나", "abc"]
SHORT_TEXTS = ONE_POSITION + TWO_POSITIONS + THREE_POSITIONS

LANES_AND_WAVES = [("pos", "2"), ("pos", "3"), ("pos8", "2"), ("pos8", "3")]
BATCH_SIZES = (1, 5, 257)      # (a block with empty lane groups: 16-lane groups take four chunks per block, 8-lane groups eight)


def short_batches():
    """every short text in one batch (lane groups of one block end after one, two and three steps while their neighbours go on), then one text of each
    length alone (a block of one working lane group)."""
    return [SHORT_TEXTS, ONE_POSITION[:1], TWO_POSITIONS[:1], THREE_POSITIONS[:1]]


def batch(sm, n):
    return mixed_texts(sm, n, 2711)


CONTAINER_LIMITS = (3, 8, 1)      # small / medium container up to 3 / 8 live incoming paths, 1 key per bucket (KAMD_CONTAINER_LIMITS, OracleKiwi.set_container_limits)


def limited_reference(path):
    """(g) a Reference whose oracle selects its path containers by CONTAINER_LIMITS.  With these limits on both sides nearly every chunk leaves the position
    steps for a node of more than 3 live incoming paths (the commonest hand-over) and goes on in the general search, which rebuilds its running live totals
    and the resumed node's live count -- 4 ... 8: medium, more: large, and the compaction branch -- from the per-node tables the steps committed
    (state offsets, counts, LIVE counts): a wrong entry there selects another container, and with 2 keys per bucket another result."""
    import oraclelib
    from pos_rounds_cases import Reference
    orc = oraclelib.OracleKiwi(path)
    orc.set_container_limits(*CONTAINER_LIMITS)
    return Reference(orc)


def limit_containers(monkeypatch):
    """the device side of CONTAINER_LIMITS; every block the engine acquires is filled with 0xCD first (KAMD_POISON), so that a table entry the steps did not
    write reads the same on every run"""
    monkeypatch.setenv("KAMD_CONTAINER_LIMITS", ",".join(str(v) for v in CONTAINER_LIMITS))
    monkeypatch.setenv("KAMD_POISON", "1")


def edge_batch():
    """the texts that take the retries (a retry stays on its position: it reads that position's records again, after the next one's were asked for) beside the
    short ones"""
    return EDGE_TEXTS + SHORT_TEXTS


# (f) one form with 27 readings: a position of 27 to 30 records -- more than one pass of 16 -- which the typo compilations of the step kernel take in two
# passes (the second pass fetches its records itself, behind the first pass's rounds)
HOMOGRAPH = "루"
HOMOGRAPH_TAGS = ("NNG", "NNP", "NNB", "NP", "NR", "XR", "VV", "VX", "VA", "MAG", "MAJ", "IC", "MM", "XPN", "XSN", "XSV", "XSA", "XSM", "JKS", "JKO", "JKB", "JX", "JC",
                  "EF", "EC", "ETN", "ETM")
HOMOGRAPH_TEXTS = ["루", "가루", "루가 루다", "하루를 루", "루루", "가나다 루 가나다"]


def homograph_model():
    """the small synthetic model + HOMOGRAPH under every tag of HOMOGRAPH_TAGS; returns the raw model's path"""
    import os
    from dataclasses import replace
    from kiwi_amd.synth import SMALL_SPEC, SynthModel
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "_data"), exist_ok=True)
    path = os.path.join(root, "_data", "small-homographs.raw")
    SynthModel(replace(SMALL_SPEC, extra_words=tuple((HOMOGRAPH, t) for t in HOMOGRAPH_TAGS))).raw.save(path)
    return path


def typo_transformer(lib):
    """the product's typo transformer with the rules of tests/typo_cases.py, prepared (continual typos on)"""
    import test_typo_product
    from typo_cases import COND, INF, RULES
    saved, test_typo_product.LIB = test_typo_product.LIB, lib      # (ProductTypo opens the module's LIB: put back at once, other tests of the process use the module)
    try:
        prod = test_typo_product.ProductTypo(1.0, INF)
    finally:
        test_typo_product.LIB = saved
    for origs, errs, cost, cond, dia in RULES:
        for o in origs:
            for e in errs:
                assert prod.add(o, e, cost, COND[cond], dia) == 0
    prod.prepare(True)
    return prod


def typo_analyze(prod):
    """`analyze` for pos_rounds_cases.check: the batch through kamd_analyze_batch_typo (threshold 2.5)"""
    import ctypes as C
    import numpy as np
    import oraclelib
    from kiwi_amd.api import Results

    def analyze(dev, texts):
        L = dev.lib
        L.kamd_analyze_batch_typo.restype = C.c_void_p
        L.kamd_analyze_batch_typo.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int]
        enc = [np.frombuffer(t.encode("utf-16-le", errors="surrogatepass"), np.uint16) for t in texts]
        offs = np.zeros(len(enc) + 1, np.uint64)
        offs[1:] = np.cumsum([len(e) for e in enc])
        flat = np.concatenate(enc)
        r = L.kamd_analyze_batch_typo(dev.h, prod.h, 2.5, 0, flat.ctypes.data, offs.ctypes.data, len(texts), 1, oraclelib.MATCH_ALL_WITH_NORMALIZING, 0, 0)
        assert r, L.kamd_last_error()
        return Results(L, r).to_python()
    return analyze


if __name__ == "__main__":
    # child of test_pos_step_head_cpu.py: HOMOGRAPH_TEXTS through the typo compilation of a KAMD_POSSTATS build of the lane emulator (argv[1]); the library
    # prints its counters and histograms when the process ends
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    from kiwi_amd.api import KiwiAmd
    prod = typo_transformer(sys.argv[1])
    dev = KiwiAmd(homograph_model(), lib_path=sys.argv[1])
    typo_analyze(prod)(dev, HOMOGRAPH_TEXTS)
    dev.close()
    prod.close()
