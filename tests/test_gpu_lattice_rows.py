"""GPU (-m gpu): the tail of k_lattice_wave on the device -- scans on the DPP path with carries between blocks of 64 ops / 64 positions, candidate records
copied from the model's row table (tests/lattice_rows_cases.py).  Small Knlm and small CoNgram model; every batch: default == oracle == general kernel ==
KAMD_LATTICE_EXPAND=0 == KAMD_LATTICE_WAVE=0."""
import os

import pytest

from lattice_rows_cases import batches, check_rows, ops_of, ops_texts
from pos_rounds_cases import NO_CUT_OFF, Reference, check
from pos_step_head_cases import batch, limit_containers, limited_reference

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SMALLCAPS = os.path.join(os.path.dirname(HERE), "kiwi_amd", "libkiwi_hip_smallcaps.so")


@pytest.fixture(scope="module")
def refs(oracle, small_cong_model):
    import oraclelib
    return {"knlm": Reference(oracle), "cong": Reference(oraclelib.OracleKiwi(small_cong_model[1]))}


def _opener(path, lib=None):
    from kiwi_amd.api import KiwiAmd
    return lambda: KiwiAmd(path, lib_path=lib)


@pytest.mark.parametrize("which", ["knlm", "cong"])
def test_chunks_of_63_64_and_65_ops_are_what_they_claim(small_model, small_cong_model, monkeypatch, capfd, which):
    """the premise of the first batch: k_lattice_wave builds each of the three texts as one chunk of exactly that many ops"""
    sm, path = small_model if which == "knlm" else small_cong_model
    monkeypatch.setenv("KAMD_LATTICE_STATS", "1")
    dev = _opener(path)()
    try:
        for k, text in ops_texts(sm).items():
            built, ops, _ = ops_of(dev, text, capfd)
            assert (built, ops) == (1, k), text
    finally:
        dev.close()


@pytest.mark.parametrize("which", ["knlm", "cong"])
def test_every_batch_equals_oracle_and_the_other_lattice_paths(refs, small_model, small_cong_model, monkeypatch, which):
    sm, path = small_model if which == "knlm" else small_cong_model
    for name, texts in batches(sm).items():
        check_rows(_opener(path), refs[which], texts, monkeypatch)
    everything = [t for texts in batches(sm).values() for t in texts]
    check_rows(_opener(path), refs[which], everything, monkeypatch)


@pytest.fixture(scope="module")
def limited_ref(small_model):
    return limited_reference(small_model[1])


def test_general_search_reads_the_rows_copied_from_the_table(limited_ref, small_model, monkeypatch):
    """tiny path containers on both sides, small-capacities build: nearly every chunk leaves the position steps and goes on in the general search, which
    reads the candidate records k_lattice_wave copied from the table into the chunk's packs"""
    assert os.path.exists(SMALLCAPS), "libkiwi_hip_smallcaps.so is not built (make -C kiwi_amd/csrc smallcaps; build() makes it)"
    sm, path = small_model
    limit_containers(monkeypatch)
    texts = batch(sm, 64) + [t for b in batches(sm).values() for t in b]
    check(_opener(path, SMALLCAPS), limited_ref, texts, monkeypatch)
    check(_opener(path, SMALLCAPS), limited_ref, texts, monkeypatch, cut_off=NO_CUT_OFF)
