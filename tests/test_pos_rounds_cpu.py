"""CPU (not gpu): the item rounds of the position-step kernel k_pos_path on the lane emulator of tests/hipemu (the library is built and loaded by path here,
as tests/test_hipemu.py does).  A round is the next up to 64 items of the four (eight) lane groups' records, whatever 16-lane rows a record falls in: the mark
map is filled along the rows and carried across them, the per-key winners come from a segmented arg-max with three cross-row carries, and a record of 17
to 64 items is an ordinary record.  Every case: device == oracle analysis for analysis, and == the general kernel alone (tests/pos_rounds_cases.py)."""
import os
import subprocess
import sys

import pytest

from corpora import EDGE_TEXTS, dictionary_mix, force_lanes, synthetic
from pos_rounds_cases import BATCH_SIZES, NO_CUT_OFF, TIGHT_CUT_OFF, Reference, check, long_texts, mixed_texts, norm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "hipemu")


@pytest.fixture(scope="module")
def emu_libs():
    subprocess.check_call(["make", "-C", EMU, "-j8"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", EMU, "smallcaps", "-j8"], stdout=subprocess.DEVNULL)
    # a build whose dead-bit window looks 32 states back instead of 256: predecessor ranges reach behind it, and the parent selection walks the arena
    # (built by tools/pos_rounds.py into an output of its own, with the developer counters)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pos_rounds
    short = pos_rounds.build("-DKAMD_TEST_DEAD_WINDOW=32", "posstats_deadwin")
    return os.path.join(EMU, "_build", "libkiwi_hipemu.so"), os.path.join(EMU, "_build", "libkiwi_hipemu_smallcaps.so"), short


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


def _opener(path, lib):
    from kiwi_amd.api import KiwiAmd
    return lambda: KiwiAmd(path, lib_path=lib)


@pytest.mark.parametrize("lanes,wps", [("pos", "2"), ("pos", "3"), ("pos8", "2"), ("pos8", "3")])
def test_batch_sizes_with_empty_groups_in_the_last_block(emu_libs, ref, small_model, monkeypatch, lanes, wps):
    sm, path = small_model
    force_lanes(monkeypatch, lanes)
    monkeypatch.setenv("KAMD_WPS", wps)
    for n in BATCH_SIZES:
        check(_opener(path, emu_libs[0]), ref, mixed_texts(sm, n, 2611), monkeypatch)


@pytest.mark.parametrize("build", [0, 1, 2], ids=["default", "smallcaps", "short-window"])
@pytest.mark.parametrize("lanes,wps", [("pos", "3"), ("pos8", "2")])
@pytest.mark.parametrize("case", ["tight", "none", "long"])
def test_cut_offs_and_long_texts(emu_libs, ref, small_model, monkeypatch, build, lanes, wps, case):
    """tight: most states die, whole predecessor ranges have few live parents.  none: nothing dies, records pass 16 items (the former big path) and straddle
    rows.  long: 400-jamo texts, state indices pass many multiples of the 256-bit dead window, the retry texts (a retry rewinds the arena under the window) in
    the same batch.  Also on the `smallcaps` build (staging of 8 states) and on the build with a window of 32 states (the selection's walk through the arena)."""
    sm, path = small_model
    force_lanes(monkeypatch, lanes)
    monkeypatch.setenv("KAMD_WPS", wps)
    if case == "long":
        check(_opener(path, emu_libs[build]), ref, long_texts(sm, 2621), monkeypatch)
    else:
        check(_opener(path, emu_libs[build]), ref, mixed_texts(sm, 64, 2611), monkeypatch, cut_off=TIGHT_CUT_OFF if case == "tight" else NO_CUT_OFF)


@pytest.mark.parametrize("lanes", ["pos", "pos8"])
def test_cong_compilation(emu_libs, small_cong_model, monkeypatch, lanes):
    import oraclelib
    sm, path = small_cong_model
    force_lanes(monkeypatch, lanes)
    monkeypatch.setenv("KAMD_WPS", "3")
    r = Reference(oraclelib.OracleKiwi(path))
    check(_opener(path, emu_libs[0]), r, mixed_texts(sm, 64, 2631), monkeypatch, cut_off=NO_CUT_OFF)


@pytest.mark.parametrize("lanes", ["pos", "pos8"])
def test_typo_compilation(emu_libs, small_model, monkeypatch, lanes):
    """The typo compilation (two passes of records per position): misspelt texts through a typo transformer, against the oracle and the general kernel."""
    import ctypes as C
    import random
    import numpy as np
    import oraclelib
    import test_typo_product
    from kiwi_amd.api import Results
    from typo_cases import COND, INF, RULES, misspell
    sm, path = small_model
    monkeypatch.setenv("KAMD_EXPERIMENTAL_TYPO", "1")
    monkeypatch.setenv("KAMD_WPS", "3")
    force_lanes(monkeypatch, lanes)
    test_typo_product.LIB = emu_libs[0]
    prod = test_typo_product.ProductTypo(1.0, INF)
    orc_t = oraclelib.OracleTypo(1.0, INF)
    for origs, errs, cost, cond, dia in RULES:
        for o in origs:
            for e in errs:
                assert prod.add(o, e, cost, COND[cond], dia) == 0
                orc_t.add(o, e, cost, COND[cond], dia)
    prod.prepare(True); orc_t.prepare(True)
    rnd = random.Random(2641)
    texts = [misspell(t, rnd, True, True) for t in synthetic(sm, 40, 2641, min_jamo=5, max_jamo=100) + dictionary_mix(sm, 16, 2642)] + EDGE_TEXTS[:20]

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

    got = check(_opener(path, emu_libs[0]), None, texts, monkeypatch, analyze=analyze)
    orc = oraclelib.OracleKiwi(path)
    for t, y in zip(texts, got):
        assert norm(orc.analyze_typo(orc_t, t, 2.5, 0)) == y, t
    prod.close()


def test_rounds_straddle_rows_take_large_records_and_skip_dead_parents(emu_libs):
    """A KAMD_POSSTATS build of the emulator (tools/pos_rounds.py, run in a child process: the counters are printed when the library is unloaded) on 64 texts of
    the small model: records did straddle a 16-lane row, records of more than 16 items went through the rounds, dead parents were skipped -- exactly the item
    lanes that used to load a pruned parent and leave --, and a step takes fewer rounds than the same build took with the packing of whole records into
    16-lane rows: the figure tools/pos_rounds.py recorded for that packing on the same texts (profiles/pos_rounds_small64_before.txt).  The build with the
    short window selects parents by walking the arena, and scores and keeps the same items."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pos_rounds
    _, c = pos_rounds.run(pos_rounds.build(), small=True)
    before = open(os.path.join(ROOT, "profiles", "pos_rounds_small64_before.txt"), encoding="utf-8").read()
    b = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)(?= |$)", re.search(r"^\[posstats\] (.*)$", before, re.M).group(1))}
    print("rounds per step", c["rounds"] / c["waveSteps"], "before", b["rounds"] / b["waveSteps"], "straddled", c["straddled"], "records of more than 16 items", c["bigRecords"],
          "dead parents skipped", c["deadParents"])
    assert c["waveSteps"] == b["waveSteps"] and c["scored"] == b["scored"] and c["kept"] == b["kept"] and c["reps"] == b["reps"]      # (the same steps score and keep the same items)
    assert c["straddled"] > 0
    assert c["bigRecords"] > 0
    assert c["deadParents"] > 0 and c["itemLanes"] + c["deadParents"] == b["itemLanes"] and c["deadParents"] == b["deadParents"]
    assert c["arenaSelects"] == 0
    assert c["rounds"] / c["waveSteps"] < b["rounds"] / b["waveSteps"]
    _, w = pos_rounds.run(emu_libs[2], small=True)
    assert w["arenaSelects"] > 0
    assert all(w[k] == c[k] for k in ("waveSteps", "rounds", "itemLanes", "deadParents", "scored", "kept", "reps"))
