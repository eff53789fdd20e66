"""CPU (not gpu): the parity cases of tests/test_gpu_lattice_rows.py on the lane emulator of tests/hipemu (the library is built and loaded by path here, as
tests/test_hipemu.py does).  This covers the candidate records copied from the model's row table; the scans of csrc/wave_scan.hpp are the __shfl_up loops on
the emulator (their DPP form is tests/test_gpu_wave_scan.py's)."""
import os
import subprocess

import pytest

from lattice_rows_cases import batches, check_rows, ops_of, ops_texts
from pos_rounds_cases import NO_CUT_OFF, Reference, check
from pos_step_head_cases import batch, limit_containers, limited_reference

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hipemu")


@pytest.fixture(scope="module")
def emu_libs():
    subprocess.check_call(["make", "-C", EMU, "-j8"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", EMU, "smallcaps", "-j8"], stdout=subprocess.DEVNULL)
    return os.path.join(EMU, "_build", "libkiwi_hipemu.so"), os.path.join(EMU, "_build", "libkiwi_hipemu_smallcaps.so")


@pytest.fixture(scope="module")
def refs(oracle, small_cong_model):
    import oraclelib
    return {"knlm": Reference(oracle), "cong": Reference(oraclelib.OracleKiwi(small_cong_model[1]))}


def _opener(path, lib):
    from kiwi_amd.api import KiwiAmd
    return lambda: KiwiAmd(path, lib_path=lib)


@pytest.mark.parametrize("which", ["knlm", "cong"])
def test_chunks_of_63_64_and_65_ops_are_what_they_claim(emu_libs, small_model, small_cong_model, monkeypatch, capfd, which):
    """the premise of the first batch: k_lattice_wave builds each of the three texts as one chunk of exactly that many ops"""
    sm, path = small_model if which == "knlm" else small_cong_model
    monkeypatch.setenv("KAMD_LATTICE_STATS", "1")
    dev = _opener(path, emu_libs[0])()
    try:
        for k, text in ops_texts(sm).items():
            built, ops, _ = ops_of(dev, text, capfd)
            assert (built, ops) == (1, k), text
    finally:
        dev.close()


@pytest.mark.parametrize("which", ["knlm", "cong"])
def test_every_batch_equals_oracle_and_the_other_lattice_paths(emu_libs, refs, small_model, small_cong_model, monkeypatch, which):
    sm, path = small_model if which == "knlm" else small_cong_model
    for name, texts in batches(sm).items():
        check_rows(_opener(path, emu_libs[0]), refs[which], texts, monkeypatch)


@pytest.fixture(scope="module")
def limited_ref(small_model):
    return limited_reference(small_model[1])


def test_general_search_reads_the_rows_copied_from_the_table(emu_libs, limited_ref, small_model, monkeypatch):
    """tiny path containers on both sides, small-capacities build: nearly every chunk leaves the position steps and goes on in the general search, which
    reads the candidate records k_lattice_wave copied from the table into the chunk's packs"""
    sm, path = small_model
    limit_containers(monkeypatch)
    texts = batch(sm, 24) + [t for b in batches(sm).values() for t in b]
    check(_opener(path, emu_libs[1]), limited_ref, texts, monkeypatch)
    check(_opener(path, emu_libs[1]), limited_ref, texts, monkeypatch, cut_off=NO_CUT_OFF)
