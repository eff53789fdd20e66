"""GPU (-m gpu): the parity cases of tests/test_pos_rounds_cpu.py on the device -- item rounds of the position-step kernel that take the next up to 64 items
whatever rows a record falls in, records of 17 to 64 items as ordinary records.  Every case: k_pos_path == oracle analysis for analysis (tokens, positions,
fp32 scores), and == the general kernel alone (KAMD_POS_PATH=0).  Small batches of the small model; 64 sentences of the benchmarked `full` model."""
import os

import pytest

from corpora import force_lanes
from pos_rounds_cases import NO_CUT_OFF, TIGHT_CUT_OFF, Reference, check, long_texts, mixed_texts

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SMALLCAPS = os.path.join(os.path.dirname(HERE), "kiwi_amd", "libkiwi_hip_smallcaps.so")


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


def _opener(path, lib=None):
    from kiwi_amd.api import KiwiAmd
    return lambda: KiwiAmd(path, lib_path=lib)


@pytest.mark.parametrize("lanes,wps", [("pos", "2"), ("pos", "3"), ("pos8", "2"), ("pos8", "3")])
def test_batch_sizes_with_empty_groups_in_the_last_block(ref, small_model, monkeypatch, lanes, wps):
    sm, path = small_model
    force_lanes(monkeypatch, lanes)
    monkeypatch.setenv("KAMD_WPS", wps)
    for n in (5, 64, 257):
        check(_opener(path), ref, mixed_texts(sm, n, 2611), monkeypatch)


@pytest.mark.parametrize("build", ["default", "smallcaps"])
@pytest.mark.parametrize("lanes,wps", [("pos", "3"), ("pos8", "2")])
@pytest.mark.parametrize("case", ["tight", "none", "long"])
def test_cut_offs_and_long_texts(ref, small_model, monkeypatch, build, lanes, wps, case):
    sm, path = small_model
    if build == "smallcaps" and not os.path.exists(SMALLCAPS):
        pytest.skip("libkiwi_hip_smallcaps.so not built (make -C kiwi_amd/csrc smallcaps)")
    lib = SMALLCAPS if build == "smallcaps" else None
    force_lanes(monkeypatch, lanes)
    monkeypatch.setenv("KAMD_WPS", wps)
    if case == "long":
        check(_opener(path, lib), ref, long_texts(sm, 2621), monkeypatch)
    else:
        check(_opener(path, lib), ref, mixed_texts(sm, 64, 2611), monkeypatch, cut_off=TIGHT_CUT_OFF if case == "tight" else NO_CUT_OFF)


def test_64_sentences_of_the_full_model(monkeypatch):
    """The benchmarked model (bench.py's default workload c2-64k), its first 64 sentences, both builds of the kernel (two and three waves per SIMD)."""
    import oraclelib
    from kiwi_amd.workloads import get_workload
    path, texts, _ = get_workload("c2-64k")
    r = Reference(oraclelib.OracleKiwi(path))
    force_lanes(monkeypatch, "pos")
    for wps in ("2", "3"):
        monkeypatch.setenv("KAMD_WPS", wps)
        check(_opener(path), r, texts[:64], monkeypatch)
