"""CPU (not gpu): the head of a position step of k_pos_path on the lane emulator of tests/hipemu (the library is built and loaded by path here, as
tests/test_hipemu.py does).  A step's records are its first loads and the fetches for the following steps stand behind them; a lane group forms the addresses of
its chunk's tables from 32-bit offsets and keeps its arena, the chunk's index and its node count in its LDS context.  Every case: device == oracle analysis for analysis, and == the general kernel alone (tests/pos_rounds_cases.py); the inputs are those of
tests/test_gpu_pos_step_head.py (tests/pos_step_head_cases.py)."""
import os
import re
import subprocess
import sys

import pytest

from corpora import force_lanes
from pos_rounds_cases import NO_CUT_OFF, Reference, check, norm
from pos_step_head_cases import (BATCH_SIZES, HOMOGRAPH_TEXTS, LANES_AND_WAVES, batch, edge_batch, homograph_model, limit_containers, limited_reference,
                                 short_batches, typo_analyze, typo_transformer)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "hipemu")


@pytest.fixture(scope="module")
def emu_libs():
    subprocess.check_call(["make", "-C", EMU, "-j8"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", EMU, "smallcaps", "-j8"], stdout=subprocess.DEVNULL)
    return os.path.join(EMU, "_build", "libkiwi_hipemu.so"), os.path.join(EMU, "_build", "libkiwi_hipemu_smallcaps.so")


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


@pytest.fixture(scope="module")
def cong_ref(small_cong_model):
    import oraclelib
    return Reference(oraclelib.OracleKiwi(small_cong_model[1]))


def _opener(path, lib):
    from kiwi_amd.api import KiwiAmd
    return lambda: KiwiAmd(path, lib_path=lib)


def _switches(monkeypatch, lanes, wps):
    force_lanes(monkeypatch, lanes)
    monkeypatch.setenv("KAMD_WPS", wps)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_texts_of_one_two_and_three_positions(emu_libs, ref, small_model, monkeypatch, lanes, wps):
    """(a) the fetches for the next step and the one after it reach past the end of the position table in the first step"""
    _switches(monkeypatch, lanes, wps)
    for texts in short_batches():
        check(_opener(small_model[1], emu_libs[0]), ref, texts, monkeypatch)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_retries_read_their_position_again(emu_libs, ref, small_model, monkeypatch, lanes, wps):
    """(b) the edge texts: a retry stays on its position after the next position's records were asked for"""
    _switches(monkeypatch, lanes, wps)
    check(_opener(small_model[1], emu_libs[0]), ref, edge_batch(), monkeypatch)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_batch_sizes_with_empty_lane_groups(emu_libs, ref, small_model, monkeypatch, lanes, wps):
    """(c) 1, 5 and 257 texts: lane groups without a chunk step along with their block"""
    sm, path = small_model
    _switches(monkeypatch, lanes, wps)
    for n in BATCH_SIZES:
        check(_opener(path, emu_libs[0]), ref, batch(sm, n), monkeypatch)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_cong_nodes_of_more_than_16_incoming_paths(emu_libs, cong_ref, small_cong_model, monkeypatch, lanes, wps):
    """(d) nothing is pruned on the small CoNgram model: nodes with more than 16 incoming paths list their contexts in the record area before the step's
    records are staged there"""
    sm, path = small_cong_model
    _switches(monkeypatch, lanes, wps)
    check(_opener(path, emu_libs[0]), cong_ref, batch(sm, 64), monkeypatch, cut_off=NO_CUT_OFF)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_hand_overs_of_the_small_capacities_build(emu_libs, ref, small_model, monkeypatch, lanes, wps):
    """(e) staging of 8 states: lane groups leave the steps with a fetch in flight and go on in the general search inside the kernel"""
    sm, path = small_model
    _switches(monkeypatch, lanes, wps)
    check(_opener(path, emu_libs[1]), ref, batch(sm, 64), monkeypatch)
    check(_opener(path, emu_libs[1]), ref, batch(sm, 64), monkeypatch, cut_off=NO_CUT_OFF)


@pytest.fixture(scope="module")
def limited_ref(small_model):
    return limited_reference(small_model[1])


@pytest.mark.parametrize("build", ["default", "smallcaps"])
@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_general_search_resumes_on_the_live_counts_the_steps_committed(emu_libs, limited_ref, small_model, monkeypatch, build, lanes, wps):
    """(g) containers of 3 / 8 paths and 2 keys per bucket on both sides: chunks leave the steps at nodes of 4 and more live incoming paths and the general search
    -- inside the kernel and in k_best_path -- takes the container of the resumed node from the per-node live counts the steps wrote"""
    sm, path = small_model
    _switches(monkeypatch, lanes, wps)
    limit_containers(monkeypatch)
    lib = emu_libs[1] if build == "smallcaps" else emu_libs[0]
    check(_opener(path, lib), limited_ref, batch(sm, 64), monkeypatch)
    check(_opener(path, lib), limited_ref, batch(sm, 64), monkeypatch, cut_off=NO_CUT_OFF)


@pytest.mark.parametrize("wps", ["2", "3"])
def test_typo_compilation_takes_a_position_of_17_to_32_records_in_two_passes(emu_libs, monkeypatch, wps):
    """(f) a form with 27 readings: its position has 27 to 30 records.  The typo compilation of the step kernel (16-lane groups) == the oracle's typo analysis
    == the general kernel; and a KAMD_POSSTATS build (tools/pos_rounds.py, run in a child process: the histograms are printed when the library is unloaded)
    shows that positions of 17 to 32 records went through the steps and that no chunk left them."""
    import oraclelib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pos_rounds
    path = homograph_model()
    monkeypatch.setenv("KAMD_EXPERIMENTAL_TYPO", "1")
    _switches(monkeypatch, "pos", wps)
    prod = typo_transformer(emu_libs[0])
    try:
        got = check(_opener(path, emu_libs[0]), None, HOMOGRAPH_TEXTS, monkeypatch, analyze=typo_analyze(prod))
    finally:
        prod.close()
    orc = oraclelib.OracleKiwi(path)
    orc_t = oraclelib.OracleTypo(1.0, float("inf"))
    from typo_cases import COND, RULES
    for origs, errs, cost, cond, dia in RULES:
        for o in origs:
            for e in errs:
                orc_t.add(o, e, cost, COND[cond], dia)
    orc_t.prepare(True)
    for t, y in zip(HOMOGRAPH_TEXTS, got):
        assert norm(orc.analyze_typo(orc_t, t, 2.5, 0)) == y, t
    env = dict(os.environ, KAMD_POS_STATS="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "pos_step_head_cases.py"), pos_rounds.build()], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    hist = {}
    for m in re.finditer(r"^\[poshist\] nRec:(.*)$", r.stderr, re.M):
        for k, v in re.findall(r"(\d+):(\d+)", m.group(1)):
            hist[int(k)] = hist.get(int(k), 0) + int(v)
    print("records per position", sorted(hist.items()))
    assert sum(v for k, v in hist.items() if 17 <= k <= 32) > 0
    assert not any(k > 32 for k in hist)
    left = re.search(r"^\[pos\] chunks (\d+) \(searched (\d+)\), carried on in the general search by the kernel itself (\d+), left to k_best_path (\d+)", r.stderr, re.M)
    assert left and left.group(1) == left.group(2) == str(len(HOMOGRAPH_TEXTS)) and left.group(3) == "0" and left.group(4) == "0", r.stderr[-2000:]
