"""CPU: the CoNgram query API's C surface -- include/kiwi_capi.h declares the reference's kiwi_cong_* functions and kiwi_similarity_pair_t exactly as
the reference's capi.h does (tests/golden/cong_query_decls.json, written from it by tools/make_golden_cong_query.py), the library exports them and the
batched kamd_cong_* forms, the order key the kernel sorts by is the documented one (score descending, -0 == +0, NaN last), and the reference
goldens of the query results (tests/golden/cong_query_<model>.json, compared with the product in tests/test_gpu_cong_query.py) still describe the
synthetic models this tree generates."""
import ctypes
import json
import os

import numpy as np
import pytest

from kiwi_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "cong_query_decls.json"), encoding="utf-8"))
KAMD_CONG = ["kamd_cong_info", "kamd_cong_topk", "kamd_cong_pairs", "kamd_cong_to_context_id", "kamd_cong_from_context_id",
             "kamd_cong_inv_norms", "kamd_cong_table"]


def _decls():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_cong_query", os.path.join(ROOT, "tools", "make_golden_cong_query.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.cong_declarations(open(os.path.join(ROOT, "include", "kiwi_capi.h"), encoding="utf-8").read())


def test_declarations_equal_the_reference():
    decls, pair = _decls()
    assert decls == GOLDEN["functions"]
    assert pair == GOLDEN["kiwi_similarity_pair_t"]


def test_symbols_exported():
    if not os.path.exists(api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(api.LIB_PATH)
    names = sorted(GOLDEN["functions"]) + KAMD_CONG
    assert set(KAMD_CONG) <= set(api.declared_symbols("kiwi_amd.h"))
    assert set(GOLDEN["functions"]) <= set(api.declared_symbols("kiwi_capi.h"))
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_pair_layout_matches_the_reference():
    class Pair(ctypes.Structure):
        _fields_ = [("id", ctypes.c_uint32), ("score", ctypes.c_float)]
    assert ctypes.sizeof(Pair) == 8 and Pair.score.offset == 4      # the reference casts a pair<uint32_t, float>* to it (src/capi/kiwi_c.cpp:1410)


@pytest.mark.parametrize("seed", [0, 1])
def test_order_key_restatement(seed):
    """flat_model.hpp congOrderKey restated: ascending keys = descending scores, and -0 / +0 one score (the reference compares with `>`)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("tgcq", os.path.join(HERE, "test_gpu_cong_query.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.standard_normal(500).astype(np.float32) * 10, np.float32([0.0, -0.0, -99999.0, 3.5, 3.5, np.inf, -np.inf, np.nan])])
    k = mod.order_key(s)
    order = np.lexsort((np.arange(len(s)), k))
    assert np.isnan(s[order[-1]])
    assert (np.diff(s[order[:-1]].astype(np.float64)) <= 0).all()
    assert k[-8] == k[-7] and k[-5] == k[-4]


@pytest.mark.parametrize("name", ["small", "global16", "vl4"])
def test_reference_goldens_match_the_synthetic_models(name):
    """The goldens were made from the cong.mdl bytes this tree's generator writes (same SHA-256), and their answers obey the reference's contracts:
    counts min(top_n, V) (0 out of range), scores in descending order, self at -99999 for similar words."""
    import hashlib
    from kiwi_amd import synth
    G = json.load(open(os.path.join(HERE, "golden", f"cong_query_{name}.json"), encoding="utf-8"))
    blob = synth.SynthModel(getattr(synth, G["model"])).raw.cong
    assert hashlib.sha256(blob).hexdigest() == G["cong_mdl_sha256"]
    V, Cn = G["vocab"], G["contexts"]
    for a in G["answers"]:
        op, q = a["q"][0], a["q"][1:]
        if op not in "WCPD":
            continue
        n = q[-1]
        valid = q[0] < (V if op == "W" else Cn)
        assert len(a["ids"]) == (min(n, V) if valid else 0), a["q"]
        sc = np.array([int(h, 16) for h in a["scores"]], np.uint32).view(np.float32)
        assert (np.diff(sc.astype(np.float64)) <= 0).all(), a["q"]
        if op == "W" and valid and n >= V:
            assert sc[-1] == np.float32(-99999.0)
