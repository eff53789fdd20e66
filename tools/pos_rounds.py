#!/usr/bin/env python3
"""Developer aid: how full the item rounds of k_pos_path are, counted by the lane emulator (no GPU).

Builds tests/hipemu with -DKAMD_POSSTATS into an output of its own (tests/hipemu/_build/libkiwi_hipemu_posstats.so), analyses N sentences of a
workload in a child process and prints the counter line the library writes at exit, followed by the derived figures (rounds per wavefront step, items
per round, share of the 64 lanes used).

    python tools/pos_rounds.py [--workload c2-64k] [--n 600]      the first N sentences of a bench workload (kiwi_amd/workloads.py)
    python tools/pos_rounds.py --small [--n 64]                   the small synthetic model of the test suite, texts of tests/corpora.py (seed 2601)

The outputs committed under profiles/ (pos_rounds_*.txt) are this script's, before and after a change of the packing."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu")
LIB = os.path.join(EMU, "_build", "libkiwi_hipemu_posstats.so")
SMALL_SEED = 2601


def build(extra="", tag="posstats"):
    """(extra: further defines of a test build, with a tag for its own object directory and library)"""
    lib = f"_build/libkiwi_hipemu_{tag}.so"
    subprocess.check_call(["make", "-C", EMU, "-j8", f"OBJ=_build/obj_{tag}", f"EXTRA=-DKAMD_POSSTATS {extra}".strip(), f"OUT={lib}"], stdout=subprocess.DEVNULL)
    return os.path.join(EMU, lib)


def small_texts(sm, n):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from corpora import EDGE_TEXTS, dictionary_mix, synthetic
    return (synthetic(sm, n - n // 4, SMALL_SEED, min_jamo=5, max_jamo=150) + dictionary_mix(sm, n // 4, SMALL_SEED + 1) + EDGE_TEXTS)[:n]


def child(args):
    sys.path.insert(0, ROOT)
    from kiwi_amd.api import KiwiAmd
    if args.small:
        from kiwi_amd.synth import SMALL_SPEC, SynthModel
        os.makedirs(os.path.join(ROOT, "_data"), exist_ok=True)
        path = os.path.join(ROOT, "_data", "small.raw")
        sm = SynthModel(SMALL_SPEC)
        sm.raw.save(path)
        texts = small_texts(sm, args.n)
    else:
        from kiwi_amd.workloads import get_workload
        path, texts, _ = get_workload(args.workload)
        texts = texts[:args.n]
    dev = KiwiAmd(path, lib_path=args.lib)
    dev.analyze_batch(texts).close()
    dev.close()


def counters(stderr):
    """(the lines, {name: value}) of the library's `[posstats]` lines -- one per compilation of the search (Knlm, typo, CoNgram, typo + CoNgram), summed;
    compilations that did not run and figures a line derives itself are left out."""
    total, lines = {}, []
    for m in re.finditer(r"^\[posstats\] (.*)$", stderr, re.M):
        w = m.group(1).split()
        c = {k: int(v) for k, v in zip(w[::2], w[1::2]) if v.isdigit()}
        if not c.get("waveSteps"):
            continue
        lines.append(m.group(0))
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    if not lines:
        raise RuntimeError("no [posstats] line with steps: not a KAMD_POSSTATS build, or k_pos_path did not run?\n" + stderr[-2000:])
    hand = re.findall(r"^\[pos\] chunks .*$", stderr, re.M)      # (the engine's own line with KAMD_POS_STATS=1: chunks handed over to the general search)
    return "\n".join(hand + lines), total


def run(lib, small=False, workload="c2-64k", n=None, env=None):
    n = n or (64 if small else 600)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--n", str(n)] + (["--small"] if small else ["--workload", workload])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
    return counters(r.stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2-64k")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--lib", default="")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    args.n = args.n or (64 if args.small else 600)
    if args.child:
        return child(args)
    env = dict(os.environ)
    env.setdefault("KAMD_POS_STATS", "1")      # (the engine's own line: chunks handed over to the general search)
    line, c = run(args.lib or build(), args.small, args.workload, args.n, env)
    print(f"# tools/pos_rounds.py {'--small' if args.small else '--workload ' + args.workload} --n {args.n}")
    print(line)
    steps, rounds, lanes = c["waveSteps"], c["rounds"], c["itemLanes"]
    print(f"roundsPerStep {rounds / max(steps, 1):.4f} itemsPerRound {lanes / max(rounds, 1):.2f} lanesUsed {lanes / max(rounds, 1) / 64:.3f} itemsPerStep {lanes / max(steps, 1):.2f}")


if __name__ == "__main__":
    main()
