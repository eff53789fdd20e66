"""Generates tests/golden/typo_default_sets.json: the entries of the reference's built-in typo sets (DefaultTypoSet) in the iteration order of its map,
read out of the real reference through oracle/ref_bridge.cpp (refbridge.default_typo_entries).  Run where oracle/_ref is built; the JSON is committed and
read by oracle/oraclelib.py (OracleKiwi.dialect_typo), so that the oracle's copy of the `dialect` set does not need the reference library."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import refbridge  # noqa: E402

INF = float("inf")


def _num(x):
    return None if x == INF else x


SETS = ("dialect",)      # the sets the oracle reads without the reference (OracleKiwi.dialect_typo)

sets = {}
for name in SETS:
    entries, continual, lengthening = refbridge.default_typo_entries(name)
    sets[name] = {"continual": _num(continual), "lengthening": _num(lengthening),
                  "entries": [[orig, err, _num(cost), cond, dia] for orig, err, cost, cond, dia in entries]}
out = os.path.join(ROOT, "tests", "golden", "typo_default_sets.json")
doc = json.dumps({"reference": "bab2min/Kiwi v0.23.1 src/TypoTransformer.cpp via oracle/ref_bridge.cpp (kref_typo_default_entries); costs null = infinite",
                  "entry": ["orig", "error", "cost", "cond", "dialect"], "sets": sets}, ensure_ascii=False, separators=(",", ":"))
with open(out, "w", encoding="utf-8") as f:
    f.write(doc.replace("],[", "],\n[") + "\n")      # one entry per line
print(out, {k: len(v["entries"]) for k, v in sets.items()})
