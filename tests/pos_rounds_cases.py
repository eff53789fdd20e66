"""Shared by tests/test_pos_rounds_cpu.py (lane emulator) and tests/test_gpu_pos_rounds.py (device): the inputs and the comparison of the parity cases for the
item rounds of the position-step kernel -- a round is the next up to 64 items whatever 16-lane rows a record falls in, a record of 17 to 64 items is an
ordinary record.  Every case compares analysis for analysis (tokens, positions, fp32 scores) with the CPU oracle and with the general search kernel
(KAMD_POS_PATH=0) of the same library."""
import os
from dataclasses import astuple

from corpora import EDGE_TEXTS, dictionary_mix, synthetic

TIGHT_CUT_OFF = 2.0        # most states die: predecessor ranges with few live parents, nodes that keep one state
NO_CUT_OFF = 1.0e9         # nothing dies: records of more than 16 items (the former big path), containers up to the hand-over limit
BATCH_SIZES = (1, 4, 5, 64, 257)      # (a last block with empty lane groups: 16-lane groups take four chunks per block, 8-lane groups eight)


def norm(res):
    return [([astuple(t) for t in a[0]], a[1]) for a in res]


def mixed_texts(sm, n, seed):
    """synthetic 5-150 jamo + dictionary mix + the edge texts, n of them (the edge texts in every batch that has room for them)."""
    k = max(0, n - len(EDGE_TEXTS))
    t = synthetic(sm, k - k // 3, seed, min_jamo=5, max_jamo=150) + dictionary_mix(sm, k // 3, seed + 1) + EDGE_TEXTS
    return t[-n:] if n < len(t) else t


def long_texts(sm, seed, n=6):
    """Texts of 400 jamo -- state indices run far past the LDS ring of recent states and past many multiples of 256 -- with the edge texts (the ones that take the
    retries among them) in the same batch."""
    return synthetic(sm, n, seed, min_jamo=400, max_jamo=400) + EDGE_TEXTS


class Reference:
    """Oracle analyses, computed once per (configuration, text) and shared by the cases."""
    def __init__(self, orc):
        self.orc, self.cache = orc, {}

    def get(self, texts, cut_off=None):
        miss = [s for s in dict.fromkeys(texts) if (cut_off, s) not in self.cache]
        if miss:
            try:
                if cut_off is not None:
                    self.orc.set_config(cut_off=cut_off)
                for s in miss:
                    self.cache[(cut_off, s)] = norm(self.orc.analyze(s))
            finally:
                self.orc.set_config()
        return [self.cache[(cut_off, s)] for s in texts]


def check(make_dev, ref, texts, monkeypatch, cut_off=None, analyze=None):
    """`make_dev()` opens the library under test with the environment as it is.  Position-step kernel == oracle, and == the general kernel alone."""
    analyze = analyze or (lambda dev, t: dev.analyze_batch(t).to_python())
    dev = make_dev()
    try:
        if cut_off is not None:
            dev.set_config(cut_off=cut_off)
        got = [norm(y) for y in analyze(dev, texts)]
    finally:
        dev.close()
    if ref is not None:
        want = ref.get(texts, cut_off)
        for s, w, y in zip(texts, want, got):
            assert w == y, (cut_off, s)
    before = os.environ.get("KAMD_POS_PATH")
    monkeypatch.setenv("KAMD_POS_PATH", "0")
    try:
        gen = make_dev()
        try:
            if cut_off is not None:
                gen.set_config(cut_off=cut_off)
            general = [norm(y) for y in analyze(gen, texts)]
        finally:
            gen.close()
    finally:
        if before is None:
            monkeypatch.delenv("KAMD_POS_PATH")
        else:
            monkeypatch.setenv("KAMD_POS_PATH", before)
    for s, g, y in zip(texts, general, got):
        assert g == y, (cut_off, s)
    return got
