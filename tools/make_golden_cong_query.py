#!/usr/bin/env python3
"""Goldens of the CoNgram query API, made from the reference (build box only; fixtures under tests/golden/):

  tests/golden/cong_query_decls.json    the reference header's declarations of the kiwi_cong_* functions (eight) and of kiwi_similarity_pair_t
                                        (include/kiwi/capi.h), whitespace-normalised: tests/test_cong_query_cpu.py holds include/kiwi_capi.h to them
  tests/golden/cong_query_<model>.json  what the reference's CoNgramModel answers (tools/cong_query_ref.cpp, linked with oracle/_ref/libkiwi_ref_x86.so
                                        from `make -C oracle refx86`) on the synthetic cong.mdl of SMALL_CONG_SPEC, SMALL_CONG_GLOBAL16_SPEC and
                                        MID_CONG_VL4_SPEC: fixed query sets of every function, with the SHA-256 of the cong.mdl bytes (a test tells a
                                        drifted synthetic model from a wrong answer)

    python tools/make_golden_cong_query.py [REFERENCE_ROOT]"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def normalise(decl):
    decl = re.sub(r"\bDECL_DLL\b", "", decl)
    decl = re.sub(r"\s+", " ", decl).strip()
    return re.sub(r"\s*([(),*;])\s*", r"\1", decl)


def cong_declarations(header_text):
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    decls = {m.group(2): normalise(m.group(0)) for m in re.finditer(r"(DECL_DLL\s+)?[A-Za-z_][\w ]*?\**\s*\b(kiwi_cong_\w+)\s*\([^;]*\)\s*;", text)}
    pair = re.search(r"typedef\s+struct\s*\{[^}]*\}\s*kiwi_similarity_pair_t\s*;", text)
    return decls, normalise(pair.group(0)) if pair else None


MODELS = {"small": "SMALL_CONG_SPEC", "global16": "SMALL_CONG_GLOBAL16_SPEC", "vl4": "MID_CONG_VL4_SPEC"}


def build_shim(ref):
    import subprocess
    lib = os.path.join(ROOT, "oracle", "_ref", "libkiwi_ref_x86.so")
    assert os.path.exists(lib), "run `make -C oracle refx86` first"
    exe = os.path.join(ROOT, "tools", "_build", "cong_query_ref")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-DKIWI_ARCH_X86_64", "-I" + os.path.join(ref, "include"), os.path.join(ROOT, "tools", "cong_query_ref.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


def queries(V, C, seed):
    """The fixed query set of one model: (kind, args) tuples in the shim's line format."""
    import numpy as np
    rng = np.random.default_rng(seed)
    q = []
    for n in (10,) * 24 + (300,) * 2:
        q.append(("W", int(rng.integers(0, V)), n))
        if C >= V:      # (C < V: the reference's mostSimilarContexts writes past its buffer)
            q.append(("C", int(rng.integers(0, C)), n))
        q.append(("P", int(rng.integers(0, C)), n))
        q.append(("D", int(rng.integers(0, C)), int(rng.integers(0, C)), float(rng.choice([0.25, 0.5, 1.0, 1.5])), n))
    q += [("W", V, 5), ("P", C, 5)]
    for _ in range(60):
        q.append(("S", int(rng.integers(0, V)), int(rng.integers(0, V))))
        q.append(("T", int(rng.integers(0, C)), int(rng.integers(0, C))))
    for _ in range(120):
        k = int(rng.integers(1, 5))
        q.append(("X",) + tuple(int(x) for x in rng.integers(0, V, k)))
    return q


def run_model(exe, name):
    import hashlib
    import struct
    import subprocess
    import tempfile
    import numpy as np
    sys.path.insert(0, ROOT)
    from kiwi_amd import synth
    blob = synth.SynthModel(getattr(synth, MODELS[name])).raw.cong
    V, C = struct.unpack_from("<QQ", blob)
    qs = queries(V, C, 7 + len(name))
    lines = []
    for q in qs:
        lines.append(" ".join([q[0], str(len(q) - 1)] + [str(x) for x in q[1:]]) if q[0] == "X" else " ".join(str(x) for x in q))
    lines.append("M")
    with tempfile.NamedTemporaryFile(suffix=".mdl") as f:
        f.write(blob)
        f.flush()
        out = subprocess.run([exe, f.name], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    answers = []
    for q, line in zip(qs, out):
        if q[0] in "WCPD":
            v = line.split()
            answers.append({"q": list(q), "ids": [int(x) for x in v[1::2]], "scores": v[2::2]})
        elif q[0] in "ST":
            answers.append({"q": list(q), "score": line.strip()})
        else:
            answers.append({"q": list(q), "context": int(line)})
    m = out[len(qs):]
    assert int(m[0]) == C
    rng = np.random.default_rng(99)
    sample = sorted(set(int(x) for x in rng.integers(1, C, 300)) | {1, 2, C - 1})
    cmap = {}
    for c in sample:
        v = [int(x) for x in m[1 + c].split()]
        assert v[0] == c and len(v) == 2 + v[1]
        cmap[str(c)] = v[2:]
    return {"model": MODELS[name], "cong_mdl_sha256": hashlib.sha256(blob).hexdigest(), "vocab": V, "contexts": C,
            "answers": answers, "context_word_map": cmap}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    decls, pair = cong_declarations(open(os.path.join(ref, "include", "kiwi", "capi.h"), encoding="utf-8").read())
    assert len(decls) == 8 and pair, (sorted(decls), pair)
    out = os.path.join(ROOT, "tests", "golden", "cong_query_decls.json")
    with open(out, "w", encoding="utf-8") as f:
        json.dump({"source": "include/kiwi/capi.h (Kiwi v0.23.1)", "functions": dict(sorted(decls.items())), "kiwi_similarity_pair_t": pair}, f, indent=1)
        f.write("\n")
    print("wrote", out)
    exe = build_shim(ref)
    for name in MODELS:
        out = os.path.join(ROOT, "tests", "golden", f"cong_query_{name}.json")
        with open(out, "w", encoding="utf-8") as f:
            json.dump(run_model(exe, name), f, separators=(",", ":"))
            f.write("\n")
        print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
