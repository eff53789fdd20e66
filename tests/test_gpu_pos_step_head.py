"""GPU (-m gpu): the parity cases of tests/test_pos_step_head_cpu.py on the device -- the head of a position step of k_pos_path: a step's records are its first
loads, the fetches for the following steps stand behind them, and a lane group forms the addresses of its chunk's tables from 32-bit offsets.  Every case:
k_pos_path == oracle analysis for analysis (tokens, positions, fp32 scores), and == the general kernel alone (KAMD_POS_PATH=0).  Small models, small batches;
16-lane and 8-lane groups, the builds for two and for three waves per SIMD."""
import os

import pytest

from corpora import force_lanes
from pos_rounds_cases import NO_CUT_OFF, Reference, check
from pos_step_head_cases import BATCH_SIZES, LANES_AND_WAVES, batch, edge_batch, limit_containers, limited_reference, short_batches

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SMALLCAPS = os.path.join(os.path.dirname(HERE), "kiwi_amd", "libkiwi_hip_smallcaps.so")


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


@pytest.fixture(scope="module")
def cong_ref(small_cong_model):
    import oraclelib
    return Reference(oraclelib.OracleKiwi(small_cong_model[1]))


def _opener(path, lib=None):
    from kiwi_amd.api import KiwiAmd
    return lambda: KiwiAmd(path, lib_path=lib)


def _switches(monkeypatch, lanes, wps):
    force_lanes(monkeypatch, lanes)
    monkeypatch.setenv("KAMD_WPS", wps)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_texts_of_one_two_and_three_positions(ref, small_model, monkeypatch, lanes, wps):
    """(a) the fetches for the next step and the one after it reach past the end of the position table in the first step"""
    _switches(monkeypatch, lanes, wps)
    for texts in short_batches():
        check(_opener(small_model[1]), ref, texts, monkeypatch)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_retries_read_their_position_again(ref, small_model, monkeypatch, lanes, wps):
    """(b) the edge texts: a retry stays on its position after the next position's records were asked for"""
    _switches(monkeypatch, lanes, wps)
    check(_opener(small_model[1]), ref, edge_batch(), monkeypatch)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_batch_sizes_with_empty_lane_groups(ref, small_model, monkeypatch, lanes, wps):
    """(c) 1, 5 and 257 texts: lane groups without a chunk step along with their block"""
    sm, path = small_model
    _switches(monkeypatch, lanes, wps)
    for n in BATCH_SIZES:
        check(_opener(path), ref, batch(sm, n), monkeypatch)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_cong_nodes_of_more_than_16_incoming_paths(cong_ref, small_cong_model, monkeypatch, lanes, wps):
    """(d) nothing is pruned on the small CoNgram model: nodes with more than 16 incoming paths list their contexts in the record area before the step's
    records are staged there"""
    sm, path = small_cong_model
    _switches(monkeypatch, lanes, wps)
    check(_opener(path), cong_ref, batch(sm, 64), monkeypatch, cut_off=NO_CUT_OFF)


@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_hand_overs_of_the_small_capacities_build(ref, small_model, monkeypatch, lanes, wps):
    """(e) staging of 8 states: lane groups leave the steps with a fetch in flight and go on in the general search inside the kernel"""
    assert os.path.exists(SMALLCAPS), "libkiwi_hip_smallcaps.so is not built (make -C kiwi_amd/csrc smallcaps; build() makes it)"
    sm, path = small_model
    _switches(monkeypatch, lanes, wps)
    check(_opener(path, SMALLCAPS), ref, batch(sm, 64), monkeypatch)
    check(_opener(path, SMALLCAPS), ref, batch(sm, 64), monkeypatch, cut_off=NO_CUT_OFF)


@pytest.fixture(scope="module")
def limited_ref(small_model):
    return limited_reference(small_model[1])


@pytest.mark.parametrize("build", ["default", "smallcaps"])
@pytest.mark.parametrize("lanes,wps", LANES_AND_WAVES)
def test_general_search_resumes_on_the_live_counts_the_steps_committed(limited_ref, small_model, monkeypatch, build, lanes, wps):
    """(g) containers of 3 / 8 paths and 2 keys per bucket on both sides: chunks leave the steps at nodes of 4 and more live incoming paths and the general search
    -- inside the kernel and in k_best_path -- takes the container of the resumed node from the per-node live counts the steps wrote"""
    sm, path = small_model
    _switches(monkeypatch, lanes, wps)
    limit_containers(monkeypatch)
    lib = SMALLCAPS if build == "smallcaps" else None
    if build == "smallcaps":
        assert os.path.exists(SMALLCAPS), "libkiwi_hip_smallcaps.so is not built (make -C kiwi_amd/csrc smallcaps; build() makes it)"
    check(_opener(path, lib), limited_ref, batch(sm, 64), monkeypatch)
    check(_opener(path, lib), limited_ref, batch(sm, 64), monkeypatch, cut_off=NO_CUT_OFF)
