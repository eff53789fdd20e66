"""GPU (-m gpu): the CoNgram query API (kiwi_amd/csrc/cong_query_kernel.hip; kamd_cong_* and the reference's kiwi_cong_* functions) against a numpy
restatement of the reference's formulas (src/CoNgramModel.cpp:2416-2745) over the product's own tables and row norms: every kind bit for bit, in the
deterministic order (score descending, then id ascending).  Plus the C ABI's edge cases, batched == single calls, the context maps, and queries beside
analyses on one handle."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from corpora import synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_W, KIND_C, KIND_P, KIND_D = 0, 1, 2, 3


@pytest.fixture(scope="module")
def small_cong_global16_model():
    from kiwi_amd.synth import SynthModel, SMALL_CONG_GLOBAL16_SPEC
    d = os.path.join(ROOT, "_data")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "small-cong-global16.raw")
    sm = SynthModel(SMALL_CONG_GLOBAL16_SPEC)
    sm.raw.save(path)
    return sm, path


@pytest.fixture(scope="module", params=["small", "global16", "vl4"])
def cong_engine(request):
    from kiwi_amd.api import KiwiAmd
    fixture = {"small": "small_cong_model", "global16": "small_cong_global16_model", "vl4": "mid_cong_vl4_model"}[request.param]
    sm, path = request.getfixturevalue(fixture)
    eng = KiwiAmd(path, lm_mode=3)
    yield request.param, path, eng, Restated(eng)
    eng.close()


def order_key(s):
    s = np.where(s == 0, np.float32(0), s).astype(np.float32)
    u = s.view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0xFFFFFFFF), ~u)      # NaN after every number


class Restated:
    """The four score formulas in fp32, one rounding per operation in the reference's order (numpy float32 arithmetic is correctly rounded)."""

    def __init__(self, eng):
        self.V, self.C, self.dim = eng.cong_info()
        self.out, self.out_sc, _ = eng.cong_table(False)
        self.ctx, self.ctx_sc, self.ctx_bias = eng.cong_table(True)
        self.inv_out, self.inv_ctx = eng.cong_inv_norms(False), eng.cong_inv_norms(True)
        self.out64 = self.out.astype(np.int64)
        self.ctx64 = self.ctx.astype(np.int64)

    def n_cand(self, kind):
        return min(self.V, self.C) if kind == KIND_C else self.V

    def scores(self, kind, q, bg=0, w=0.0):
        f = np.float32
        if kind == KIND_W:
            dot = (self.out64 @ self.out64[q]).astype(f)
            s = dot * self.out_sc[q] * self.out_sc
            s = s * (self.inv_out[q] * self.inv_out)
            s[q] = f(-99999.0)
        elif kind == KIND_C:
            n = self.n_cand(kind)
            dot = (self.ctx64[:n] @ self.ctx64[q]).astype(f)
            s = dot * self.ctx_sc[q] * self.ctx_sc[:n]
            s = s * (self.inv_ctx[q] * self.inv_ctx[:n])
            if q < n:
                s[q] = f(-99999.0)
        elif kind == KIND_P:
            dot = (self.out64 @ self.ctx64[q]).astype(f)
            s = dot * self.ctx_sc[q] * self.out_sc + self.ctx_bias[q]
        else:
            w = f(w)
            sc = (self.out64 @ self.ctx64[q]).astype(f) * self.ctx_sc[q] * self.out_sc
            sb = (self.out64 @ self.ctx64[bg]).astype(f) * self.ctx_sc[bg] * self.out_sc
            bias = self.ctx_bias[q] - self.ctx_bias[bg] * w
            s = (sc - sb * w) + bias
        return s.astype(f)

    def topk(self, kind, q, top_n, bg=0, w=0.0):
        s = self.scores(kind, q, bg, w)
        order = np.lexsort((np.arange(len(s)), order_key(s)))[:min(top_n, len(s))]
        return order.astype(np.uint32), s[order]


def _queries(R, kind, n, seed):
    rng = np.random.default_rng(seed)
    hi = R.V if kind == KIND_W else R.C
    ids = rng.integers(0, hi, n).astype(np.uint32)
    bg = rng.integers(0, R.C, n).astype(np.uint32)
    w = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 1.5], np.float32), n)
    return ids, bg, w


@pytest.mark.parametrize("kind", [KIND_W, KIND_C, KIND_P, KIND_D])
def test_topk_bit_exact_vs_restatement(cong_engine, kind):
    name, _, eng, R = cong_engine
    cases = [(1, 10), (7, 1), (7, 256), (7, 257), (64, 10), (3, R.V), (3, R.V + 5), (4096, 10)]
    for n, top_n in cases:
        ids, bg, w = _queries(R, kind, n, 1000 * kind + n + top_n)
        got_ids, got_sc, counts = eng.cong_topk(kind, ids, top_n, bg, w)
        check = range(n) if n <= 64 else np.random.default_rng(5).choice(n, 48, replace=False)
        for q in check:
            want_ids, want_sc = R.topk(kind, int(ids[q]), top_n, int(bg[q]), float(w[q]))
            assert counts[q] == len(want_ids), (name, kind, n, top_n, q)
            c = counts[q]
            assert np.array_equal(got_ids[q, :c], want_ids), (name, kind, n, top_n, q)
            assert np.array_equal(got_sc[q, :c].view(np.uint32), want_sc.view(np.uint32)), (name, kind, n, top_n, q)


def test_pairs_bit_exact_and_nan(cong_engine):
    name, _, eng, R = cong_engine
    rng = np.random.default_rng(11)
    for kind, hi in ((KIND_W, R.V), (KIND_C, R.C)):
        a = rng.integers(0, hi, 200).astype(np.uint32)
        b = rng.integers(0, hi, 200).astype(np.uint32)
        a[:3] = [hi, 0, hi + 7]
        b[:3] = [0, hi, 1]
        got = eng.cong_pairs(kind, a, b)
        assert np.isnan(got[:3]).all()
        for i in range(3, 200):
            s = R.scores(kind, int(a[i])) if kind == KIND_W else None
            if kind == KIND_W:
                want = s[b[i]] if a[i] != b[i] else None
            else:
                x = np.float32(int(R.ctx64[a[i]] @ R.ctx64[b[i]])) * R.ctx_sc[a[i]] * R.ctx_sc[b[i]]
                want = x * (R.inv_ctx[a[i]] * R.inv_ctx[b[i]])
            if want is not None:
                assert np.float32(got[i]).view(np.uint32) == np.float32(want).view(np.uint32), (name, kind, i)


def test_context_maps_round_trip(cong_engine):
    name, _, eng, R = cong_engine
    # variable-length keys: the reference decodes a two-key id as (high << 10) | low without adding tMax back (src/CoNgramModel.cpp:2773-2777), so an
    # element x of a sequence may stand for the id tMax + x -- one of those readings walks back to the context
    tmax = 65536 - 2048 if name == "vl4" else None
    checked = 0
    for c in range(1, R.C, max(1, R.C // 300)):
        for seq in eng.cong_from_context_id(c):
            assert len(seq) >= 1
            readings = [seq]
            if tmax is not None:
                for j in range(len(seq)):
                    readings += [np.concatenate([r[:j], [tmax + r[j]], r[j + 1:]]).astype(np.uint32) for r in readings if r[j] < (1 << 20)]
            assert any(eng.cong_to_context_id(r) == c for r in readings), (name, c, seq)
            checked += 1
    assert checked > 50
    assert eng.cong_to_context_id(np.zeros(0, np.uint32)) == 0


def _capi():
    from kiwi_amd import api
    L = C.CDLL(api.LIB_PATH)

    class Pair(C.Structure):
        _fields_ = [("id", C.c_uint32), ("score", C.c_float)]
    L.kiwi_init.restype = C.c_void_p
    L.kiwi_init.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.kiwi_close.argtypes = [C.c_void_p]
    L.kiwi_error.restype = C.c_char_p
    for f in ("kiwi_cong_most_similar_words", "kiwi_cong_most_similar_contexts", "kiwi_cong_predict_words_from_context"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_uint, C.POINTER(Pair), C.c_int]
    L.kiwi_cong_predict_words_from_context_diff.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_float, C.POINTER(Pair), C.c_int]
    for f in ("kiwi_cong_similarity", "kiwi_cong_context_similarity"):
        getattr(L, f).restype = C.c_float
        getattr(L, f).argtypes = [C.c_void_p, C.c_uint, C.c_uint]
    L.kiwi_cong_to_context_id.restype = C.c_uint
    L.kiwi_cong_to_context_id.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.c_int]
    L.kiwi_cong_from_context_id.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_uint), C.c_int]
    return L, Pair


def _single(L, Pair, k, kind, q, top_n, bg=0, w=0.0):
    buf = (Pair * max(top_n, 1))()
    if kind == KIND_W:
        n = L.kiwi_cong_most_similar_words(k, q, buf, top_n)
    elif kind == KIND_C:
        n = L.kiwi_cong_most_similar_contexts(k, q, buf, top_n)
    elif kind == KIND_P:
        n = L.kiwi_cong_predict_words_from_context(k, q, buf, top_n)
    else:
        n = L.kiwi_cong_predict_words_from_context_diff(k, q, bg, w, buf, top_n)
    return n, [(buf[i].id, buf[i].score) for i in range(max(n, 0))]


def test_capi_single_equals_batched_and_edges(cong_engine):
    from kiwi_amd.api import KiwiAmd
    _, path, _, _ = cong_engine
    L, Pair = _capi()
    k = L.kiwi_init(path.encode(), 0, 0x0400, 0)
    assert k, L.kiwi_error()
    eng = KiwiAmd(path, lm_mode=3)
    R = Restated(eng)
    for kind in (KIND_W, KIND_C, KIND_P, KIND_D):
        ids, bg, w = _queries(R, kind, 16, 77 + kind)
        got_ids, got_sc, counts = eng.cong_topk(kind, ids, 12, bg, w)
        for q in range(16):
            n, pairs = _single(L, Pair, k, kind, int(ids[q]), 12, int(bg[q]), float(w[q]))
            assert n == counts[q]
            assert [p[0] for p in pairs] == list(got_ids[q, :n])
            assert np.array_equal(np.array([p[1] for p in pairs], np.float32).view(np.uint32), got_sc[q, :n].view(np.uint32))
    # out-of-range ids: 0 results; top_n 0: 0; negative top_n: KIWIERR_FAIL with a message
    assert _single(L, Pair, k, KIND_W, R.V, 5)[0] == 0
    assert _single(L, Pair, k, KIND_P, R.C, 5)[0] == 0
    assert _single(L, Pair, k, KIND_D, 1, 5, bg=R.C)[0] == 0
    assert _single(L, Pair, k, KIND_W, 3, 0)[0] == 0
    assert L.kiwi_cong_most_similar_words(k, 3, None, -1) == -1 and L.kiwi_error()
    assert L.kiwi_cong_most_similar_words(None, 3, None, 5) == -2
    # every word when top_n >= V: the word itself last, at -99999
    n, pairs = _single(L, Pair, k, KIND_W, 5, R.V + 3)
    assert n == R.V and pairs[-1] == (5, -99999.0)
    # similar contexts: candidates [0, min(V, C)), count capped by it
    n, pairs = _single(L, Pair, k, KIND_C, 2, max(R.C, R.V) + 10)
    assert n == min(R.V, R.C) and max(p[0] for p in pairs) < min(R.V, R.C)
    assert np.isnan(L.kiwi_cong_similarity(k, R.V, 0)) and np.isnan(L.kiwi_cong_context_similarity(k, 0, R.C))
    assert L.kiwi_cong_similarity(k, 1, 2) == eng.cong_pairs(0, [1], [2])[0]
    # the context maps through the C ABI
    arr = (C.c_uint * 3)(1, 2, 3)
    assert L.kiwi_cong_to_context_id(k, arr, 3) == eng.cong_to_context_id([1, 2, 3])
    assert L.kiwi_cong_to_context_id(k, arr, 0) == 0
    for c in (1, 2, R.C - 1):
        want = np.concatenate([np.append(s, 0xFFFFFFFF) for s in eng.cong_from_context_id(c)])[:-1] if eng.cong_from_context_id(c) else np.zeros(0)
        buf = (C.c_uint * 64)()
        n = L.kiwi_cong_from_context_id(k, c, buf, 64)
        assert n == min(len(want), 64) and list(buf[:n]) == [int(x) for x in want[:n]]
    assert L.kiwi_cong_from_context_id(k, R.C, (C.c_uint * 4)(), 4) == -1 and L.kiwi_error()
    L.kiwi_close(k)
    eng.close()


def test_first_query_of_a_fresh_handle_is_a_prediction(small_cong_model):
    """The row norms reach the device with the first query of ANY kind: a handle whose first call predicts still answers similarity queries right."""
    from kiwi_amd.api import KiwiAmd
    _, path = small_cong_model
    L, Pair = _capi()
    k = L.kiwi_init(path.encode(), 0, 0x0400, 0)
    assert k, L.kiwi_error()
    n, _ = _single(L, Pair, k, KIND_P, 3, 10)
    assert n == 10
    n, _ = _single(L, Pair, k, KIND_D, 3, 10, bg=4, w=0.5)
    assert n == 10
    eng = KiwiAmd(path, lm_mode=3)
    R = Restated(eng)
    for kind, q in ((KIND_W, 5), (KIND_W, 77), (KIND_C, 2), (KIND_C, 41)):
        n, pairs = _single(L, Pair, k, kind, q, 20)
        want_ids, want_sc = R.topk(kind, q, 20)
        assert [p[0] for p in pairs] == list(want_ids), (kind, q)
        assert np.array_equal(np.array([p[1] for p in pairs], np.float32).view(np.uint32), want_sc.view(np.uint32)), (kind, q)
    eng.close()
    L.kiwi_close(k)


def test_capi_knlm_handle_fails(small_cong_model):
    _, path = small_cong_model
    L, Pair = _capi()
    k = L.kiwi_init(path.encode(), 0, 0x0200, 0)      # KIWI_BUILD_MODEL_TYPE_KNLM: no CoNgram model behind the handle
    assert k, L.kiwi_error()
    buf = (Pair * 4)()
    assert L.kiwi_cong_most_similar_words(k, 1, buf, 4) == -1
    assert b"CoNgram" in L.kiwi_error()
    assert L.kiwi_cong_predict_words_from_context_diff(k, 1, 2, 0.5, buf, 4) == -1
    assert np.isnan(L.kiwi_cong_similarity(k, 1, 2)) and np.isnan(L.kiwi_cong_context_similarity(k, 1, 2))
    assert L.kiwi_cong_to_context_id(k, (C.c_uint * 1)(1), 1) == 0
    assert L.kiwi_cong_from_context_id(k, 1, (C.c_uint * 4)(), 4) == -1
    L.kiwi_close(k)


def test_queries_beside_analyses(small_cong_model):
    from kiwi_amd.api import KiwiAmd
    sm, path = small_cong_model
    eng = KiwiAmd(path, lm_mode=3)
    texts = synthetic(sm, 3000, 4242, min_jamo=5, max_jamo=120)
    want = eng.analyze_batch(texts).to_python()
    R = Restated(eng)
    ids, bg, w = _queries(R, KIND_P, 256, 9)
    want_q = eng.cong_topk(KIND_P, ids, 10)
    got, errs = {}, []

    def analyse():
        try:
            got["a"] = [eng.analyze_batch(texts).to_python() for _ in range(3)]
        except Exception as e:      # noqa: BLE001 (reported below)
            errs.append(e)

    def query():
        try:
            got["q"] = [eng.cong_topk(KIND_P, ids, 10) for _ in range(20)]
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=analyse), threading.Thread(target=query)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert all(a == want for a in got["a"])
    assert all(all(np.array_equal(x, y) for x, y in zip(r, want_q)) for r in got["q"])
    eng.close()


def test_c_client_against_the_header(small_cong_model, tmp_path):
    """A C program using all eight kiwi_cong_* functions, compiled with gcc against include/kiwi_capi.h and linked with the product library."""
    import subprocess
    from kiwi_amd import api
    _, path = small_cong_model
    src = tmp_path / "cong_client.c"
    src.write_text(r'''
#include <math.h>
#include <stdio.h>
#include "kiwi_capi.h"
int main(int argc, char** argv)
{
    kiwi_h k = kiwi_init(argv[1], 0, KIWI_BUILD_MODEL_TYPE_CONG, 0);
    if (!k) { printf("init failed\n"); return 1; }
    kiwi_similarity_pair_t p[5];
    unsigned int ids[2] = { 1, 2 }, seq[16];
    int a = kiwi_cong_most_similar_words(k, 1, p, 5), b = kiwi_cong_most_similar_contexts(k, 1, p, 5);
    int c = kiwi_cong_predict_words_from_context(k, 1, p, 5), d = kiwi_cong_predict_words_from_context_diff(k, 1, 2, 0.5f, p, 5);
    float s1 = kiwi_cong_similarity(k, 1, 2), s2 = kiwi_cong_context_similarity(k, 1, 2);
    unsigned int ctx = kiwi_cong_to_context_id(k, ids, 2);
    int e = kiwi_cong_from_context_id(k, 1, seq, 16);
    printf("%d %d %d %d %d %d %u %d\n", a, b, c, d, isnan(s1), isnan(s2), ctx, e);
    kiwi_close(k);
    return 0;
}
''')
    exe = str(tmp_path / "cong_client")
    libdir = os.path.dirname(api.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + libdir, "-l:libkiwi_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    a, b, c, d, n1, n2, ctx, e = out.stdout.split()
    assert (a, b, c, d, n1, n2) == ("5", "5", "5", "5", "0", "0")
    assert int(e) >= 0


# ---- against the reference itself: tests/golden/cong_query_<model>.json (tools/make_golden_cong_query.py over tools/cong_query_ref.cpp, the reference's
# CoNgramModel in its SSE4.1 build).  Prediction scores bit for bit; cosine scores within the rsqrt bound (the reference's row norms come from
# _mm_rsqrt_ps, ours are correctly rounded: <= 2 x 1.5 x 2^-12 relative, 1e-3 here); ids equal except where scores tie (prediction) or lie inside
# that band of each other (cosine); context maps equal as sets of sequences.
COS_REL = 1e-3


def _golden(name):
    import json
    return json.load(open(os.path.join(ROOT, "tests", "golden", f"cong_query_{name}.json"), encoding="utf-8"))


def _f32(hexes):
    return np.array([int(h, 16) for h in hexes], np.uint32).view(np.float32)


def _cos_close(a, b):
    a, b = np.float64(a), np.float64(b)
    return abs(a - b) <= COS_REL * max(abs(a), abs(b)) + 1e-6


def test_against_the_reference_goldens(cong_engine):
    import hashlib
    name, path, eng, R = cong_engine
    G = _golden(name)
    from kiwi_amd import synth
    blob = synth.SynthModel(getattr(synth, G["model"])).raw.cong
    assert hashlib.sha256(blob).hexdigest() == G["cong_mdl_sha256"], "the synthetic model drifted: regenerate with tools/make_golden_cong_query.py"
    assert (R.V, R.C) == (G["vocab"], G["contexts"])
    kinds = {"W": KIND_W, "C": KIND_C, "P": KIND_P, "D": KIND_D}
    for a in G["answers"]:
        op, q = a["q"][0], a["q"][1:]
        if op in kinds:
            kind = kinds[op]
            bg, w, n = (q[1], q[2], q[3]) if op == "D" else (0, 0.0, q[1])
            got_ids, got_sc, counts = eng.cong_topk(kind, [q[0]], n, [bg], [w])
            c = int(counts[0])
            ref_ids, ref_sc = np.array(a["ids"], np.uint32), _f32(a["scores"])
            assert c == len(ref_ids), a["q"]
            gi, gs = got_ids[0, :c], got_sc[0, :c]
            if kind in (KIND_P, KIND_D):
                assert np.array_equal(gs.view(np.uint32), ref_sc.view(np.uint32)), a["q"]
                # ids modulo exactly equal scores; the last tie group may be cut at a different member
                last = ref_sc[-1] if c else None
                for v in np.unique(ref_sc):
                    g, r = set(gi[gs == v].tolist()), set(ref_ids[ref_sc == v].tolist())
                    assert g == r or (v == last and len(g) == len(r)), (a["q"], float(v))
            else:
                ref = dict(zip(ref_ids.tolist(), ref_sc.tolist()))
                got = dict(zip(gi.tolist(), gs.tolist()))
                for i in set(ref) & set(got):
                    assert _cos_close(got[i], ref[i]), (a["q"], i, got[i], ref[i])
                # an id in one list only lies inside the band of the other list's last score
                for i in set(got) ^ set(ref):
                    s = got.get(i, ref.get(i))
                    assert _cos_close(s, ref_sc[-1]) or _cos_close(s, gs[-1]), (a["q"], i, s)
        elif op in "ST":
            got = eng.cong_pairs(KIND_W if op == "S" else KIND_C, [q[0]], [q[1]])[0]
            want = _f32([a["score"]])[0]
            assert (np.isnan(got) and np.isnan(want)) or _cos_close(got, want), (a["q"], got, want)
        else:
            assert eng.cong_to_context_id(np.array(q, np.uint32)) == a["context"], a["q"]
    for c, flat in G["context_word_map"].items():
        want = set()
        cur = []
        for x in flat + [0xFFFFFFFF]:
            if x == 0xFFFFFFFF:
                if cur:
                    want.add(tuple(cur))
                cur = []
            else:
                cur.append(x)
        got = {tuple(int(x) for x in seq) for seq in eng.cong_from_context_id(int(c))}
        assert got == want, (name, c)
