"""Shared by tests/test_lattice_rows_cpu.py (lane emulator) and tests/test_gpu_lattice_rows.py (device): the inputs and the comparison of the parity cases for
the tail of k_lattice_wave -- wave-wide scans with carries between blocks of 64 ops / 64 positions, and the candidate records of a node copied from the
model's row table (ModelView::candRows) instead of being gathered per chunk.  Every batch: the engine as it is == the CPU oracle and == the general search
kernel (tests/pos_rounds_cases.py's `check`), == the same engine with the records written by k_expand_cands / k_expand_pos (KAMD_LATTICE_EXPAND=0) and == the
one-lane replay of the lattice (KAMD_LATTICE_WAVE=0), analysis for analysis (tokens, positions, fp32 scores)."""
import os
import re

from corpora import synthetic
from pos_rounds_cases import check, norm

# texts of the small models' corpus generator (both small models share the lexicon) whose chunk has exactly this many ops in k_lattice_wave: one block of 64
# ops less one, exactly one block, and one op in a second block -- the carries of the by-time and by-start passes and of the rank scan
OPS_SEED, OPS_COUNT, OPS_JAMO = 4242, 60, (20, 70)
OPS_TEXT_INDEX = {63: 35, 64: 18, 65: 49}


def ops_texts(sm):
    t = synthetic(sm, OPS_COUNT, OPS_SEED, min_jamo=OPS_JAMO[0], max_jamo=OPS_JAMO[1])
    return {k: t[i] for k, i in OPS_TEXT_INDEX.items()}


def ops_of(dev, text, capfd):
    """(chunks built by k_lattice_wave, their ops, their text units) of a batch of one text, from the statistics line of KAMD_LATTICE_STATS=1"""
    capfd.readouterr()
    dev.analyze_batch([text])
    err = capfd.readouterr().err
    m = re.search(r"\[lattice wave\] chunks \d+: built (\d+) .*; ops (\d+) in (\d+) text units", err)
    assert m, err[-2000:]
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def _cand_class(m):
    """class of a candidate in the CoNgram evaluator's order (csrc/lattice_expand.hpp candClassOf)"""
    from kiwi_amd.synth import Z_CODA, Z_SIOT
    tag = m.tag & 0x7F
    if tag == Z_CODA:
        return 0
    if tag == Z_SIOT:
        return 1
    if not m.socket:
        return 2
    return 4 if m.chunks else 3


def _forms(sm):
    raw = sm.raw
    name = {v: k for k, v in raw.form_map.items()}
    items = raw.form_cands.items() if isinstance(raw.form_cands, dict) else enumerate(raw.form_cands)
    return [(name[f], [raw.morphs[m] for m in cands]) for f, cands in items if f in name and cands]


def mixed_class_forms(sm):
    """dictionary forms with candidates of more than one class"""
    return [s for s, ms in _forms(sm) if isinstance(s, str) and len({_cand_class(m) for m in ms}) > 1]


def chunked_forms(sm, n=8):
    """forms with a pre-combined candidate of two chunks: its record carries the LM id of the second chunk"""
    return [s for s, ms in _forms(sm) if isinstance(s, str) and any(len(m.chunks) >= 2 for m in ms)][:n]


def all_partial_forms(sm, n=8):
    """forms every candidate of which is one half of a split stem: their nodes also get the unknown proper-noun record"""
    return [s for s, ms in _forms(sm) if isinstance(s, str) and len(s) > 1 and all(m.socket for m in ms)][:n]


def batches(sm):
    """name -> texts"""
    ops = ops_texts(sm)
    mixed, chunked, partial = mixed_class_forms(sm), chunked_forms(sm), all_partial_forms(sm)
    assert mixed and chunked and partial
    words = synthetic(sm, 4, 99, min_jamo=10, max_jamo=30)
    return {
        "63, 64 and 65 ops": [ops[63], ops[64], ops[65]],
        "more than 64 positions": synthetic(sm, 2, 17, exact_jamo=150) + synthetic(sm, 1, 18, exact_jamo=66),
        "inner spaces": [w.replace(" ", "  ", 1).replace(" ", "   ", 1) for w in words] + ["가나  다라   마바 사", "탭\t과  여러   공백", " 앞 뒤 "],
        "candidates of several classes": [" ".join(mixed), "김" + mixed[0] + "가 " + words[0]] + [words[1].split(" ")[0] + f for f in mixed],
        "chunked candidates": [" ".join(chunked)] + [words[2] + " " + f for f in chunked[:3]],
        "sentence-break tag": ["1. 첫째 2. 둘째 가. 항목 (1) 괄호", "가. " + words[3] + " 나. " + words[0]],
        "all-partial forms": [" ".join(partial)] + [f + "어" for f in partial[:3]] + [f + " " + words[1] for f in partial[:2]],
        "z-coda": ["앜", "했닼ㅋㅋ", "갘 낳닼 밬", words[2] + "닼"],
        "unknown only": ["뷁뷁뷁 쀍", "xyz", "뷁"],
        "one unit": ["가", "a", ".", "1"],
    }


def check_rows(make_dev, ref, texts, monkeypatch):
    """`make_dev()` opens the library under test with the environment as it is (the switches are read when an engine opens)"""
    got = check(make_dev, ref, texts, monkeypatch)
    for switch in ("KAMD_LATTICE_EXPAND", "KAMD_LATTICE_WAVE"):
        before = os.environ.get(switch)
        monkeypatch.setenv(switch, "0")
        try:
            dev = make_dev()
            try:
                other = [norm(y) for y in dev.analyze_batch(texts).to_python()]
            finally:
                dev.close()
        finally:
            if before is None:
                monkeypatch.delenv(switch)
            else:
                monkeypatch.setenv(switch, before)
        for s, o, y in zip(texts, other, got):
            assert o == y, (switch, s)
    return got
