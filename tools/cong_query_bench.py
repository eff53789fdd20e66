#!/usr/bin/env python3
"""Developer tool: queries/s of the CoNgram query API (kamd_cong_topk) on one MI355X, with the bandwidth of the table reads it implies.

    python tools/cong_query_bench.py [--model mid-cong-vl4|full-cong] [--top-n 10] [--reps 5]

Every (kind, Q) pair is timed as the median wall time of `reps` calls after one warm-up call; a Q-query call reads the query rows and all V candidate
rows (dim + 8 bytes each) once per query, so `table GB/s` = Q * V * (dim + 8) / time.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_path(name):
    if name == "full-cong":
        from kiwi_amd.workloads import get_workload
        return get_workload("c4-cong")[0]      # (the model of the c4-cong workload; generated on first use)
    from kiwi_amd.synth import SynthModel, MID_CONG_VL4_SPEC
    path = os.path.join(ROOT, "_data", "mid-cong-vl4.raw")
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        SynthModel(MID_CONG_VL4_SPEC).raw.save(path)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mid-cong-vl4")
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qs", default="1,64,4096")
    a = ap.parse_args()
    from kiwi_amd.api import KiwiAmd
    eng = KiwiAmd(model_path(a.model), lm_mode=3)
    V, Cn, dim = eng.cong_info()
    rng = np.random.default_rng(0)
    for kind, name in ((0, "similar_words"), (2, "predict")):
        for q in (int(x) for x in a.qs.split(",")):
            ids = rng.integers(0, V if kind == 0 else Cn, q).astype(np.uint32)
            eng.cong_topk(kind, ids, a.top_n)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                eng.cong_topk(kind, ids, a.top_n)
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            print(json.dumps({"model": a.model, "kind": name, "Q": q, "top_n": a.top_n, "V": V, "dim": dim, "ms": round(t * 1e3, 3),
                              "queries_per_s": round(q / t, 1), "table_GB_per_s": round(q * V * (dim + 8) / t / 1e9, 2)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
