"""Replay ``--solver-log`` dumps through the witness engine.

``myth analyze --solver-log DIR`` writes every uncached query as the SMT-LIB2
text of z3's ``Optimize.sexpr()`` (mythril/support/model.py:45-56).  This
module parses such files (mythril_amd/smt2.py), routes them the way the
drop-in ``get_model`` does — queries with ``minimize``/``maximize`` stay with z3,
formulas outside the vocabulary fall back — and searches the rest on the
device, many programs per launch.  It gives offline replays and benchmarks of
real analyses without z3 or solc.

    python -m mythril_amd.replay DIR [--budget 2^22] [--batch 64] [--explain-misses] [--witness-density]
                                     [--repair-misses]

``--explain-misses`` profiles every missed query (WitnessEngine.explain_miss)
and prints one more line for it: which conjuncts reject its candidates.
``--witness-density`` counts every searched query's witnesses
(WitnessEngine.search_all) and prints one more line for it: how many of its
candidates are witnesses, and the first of them.
``--repair-misses`` runs WitnessEngine.repair on every missed query and prints
one more line for it: repaired or not, the rounds used and the final number of
failed conjunct rows.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time
from dataclasses import dataclass, field
from typing import List, Optional

from .compiler import Unsupported


@dataclass
class Result:
    path: str
    status: str                      # "witness" | "miss" | "z3" (objectives) | "unsupported"
    index: Optional[int] = None
    values: dict = field(default_factory=dict)
    reason: str = ""
    arrays: dict = field(default_factory=dict)      # array -> {index: value} (Ackermann leaves)
    functions: dict = field(default_factory=dict)   # UF -> {args: value}
    profile: Optional[object] = None                # a miss under explain: engine.MissProfile (or the error's text)
    density: Optional[object] = None                # under density: (total, count, first index or None) (or the error's text)
    repair: Optional[object] = None                 # a miss under repair: {"witness", "rounds", "nfail"} (or the error's text)


def load(path: str):
    from .engine import prepare
    from .smt2 import parse_file
    s = parse_file(path)
    if s.minimize or s.maximize:
        return s, None, "objectives: answered by z3 (analysis/solver.py:51-101)"
    return s, prepare(s.asserts, s.ctx), ""


EXPLAIN_MAX = 1 << 16   # candidates of a miss profile


def explain_line(r: Result) -> str:
    """One line for a profiled miss: the query, how many candidates satisfied
    everything, how many conjuncts the nearest one fails, and the three most
    blocking conjuncts as number:sole/fail (c: the congruence conjuncts)."""
    name = os.path.basename(r.path)
    m = r.profile
    if m is None or isinstance(m, str):
        return f"miss {name}: no profile ({m})"
    top = []
    for j in m.blocking()[:3]:
        s, f = (m.congruence_sole, m.congruence_fail) if j < 0 else (m.sole[j], m.fail[j])
        top.append(f"{'c' if j < 0 else j}:{s}/{f}")
    return (f"miss {name}: satisfied {m.satisfied}/{m.count}, nearest fails {m.nearest_nfail}, "
            f"blocking (conjunct:sole/fail) {' '.join(top)}")


def density_line(r: Result) -> str:
    """One line for a counted query: how many of its candidates are witnesses
    (total / count) and the lowest witness index."""
    name = os.path.basename(r.path)
    d = r.density
    if d is None or isinstance(d, str):
        return f"density {name}: not counted ({d})"
    total, count, first = d
    return f"density {name}: {total} / {count} witnesses, first {'none' if first is None else first}"


REPAIR_ROUNDS = 8   # --repair-misses


def repair_line(r: Result) -> str:
    """One line for a miss WitnessEngine.repair was run on: repaired or not,
    the rounds it used and the conjunct rows the last base still fails."""
    name = os.path.basename(r.path)
    d = r.repair
    if d is None or isinstance(d, str):
        return f"miss {name}: no repair ({d})"
    return (f"miss {name}: {'repaired' if d['witness'] is not None else 'not repaired'}, rounds {d['rounds']}, "
            f"nfail {d['nfail']}")


def replay(paths: List[str], engine, batch: int = 64, explain: bool = False, density: bool = False,
           repair: int = 0, repair_count: Optional[int] = None) -> List[Result]:
    out: List[Result] = []
    pending = []
    for p in paths:
        try:
            s, q, why = load(p)
        except (Unsupported, RecursionError, ValueError, KeyError) as e:
            out.append(Result(p, "unsupported", reason=str(e)))
            continue
        if q is None:
            out.append(Result(p, "z3", reason=why))
            continue
        pending.append((p, s, q))
    for i in range(0, len(pending), batch):
        chunk = pending[i:i + batch]
        found = engine.search([q for _, _, q in chunk])
        for (p, s, q), w in zip(chunk, found):
            if w is None:
                out.append(Result(p, "miss"))
                if explain:
                    try:
                        out[-1].profile = engine.explain_miss(q, count=min(engine.budget, EXPLAIN_MAX))
                    except Exception as e:   # noqa: BLE001 - a diagnostic: the miss stands
                        out[-1].profile = f"{type(e).__name__}: {e}"
                if repair:
                    try:
                        prof = out[-1].profile if explain and not isinstance(out[-1].profile, str) else None
                        w2 = engine.repair(q, rounds=repair, count=repair_count, profile=prof)
                        out[-1].repair = {"witness": w2, **getattr(engine, "last_repair", {"rounds": 0, "nfail": 0})}
                    except Exception as e:   # noqa: BLE001 - a diagnostic: the miss stands
                        out[-1].repair = f"{type(e).__name__}: {e}"
            else:
                out.append(Result(p, "witness", w.index, dict(w.values), arrays=w.arrays, functions=w.functions))
            if density:
                try:
                    n = engine.launch_count([q])
                    some, total = engine.search_all(q, 1, count=n)
                    out[-1].density = (total, n, some[0].index if some else None)
                except Exception as e:   # noqa: BLE001 - a diagnostic: the result stands
                    out[-1].density = f"{type(e).__name__}: {e}"
    order = {p: k for k, p in enumerate(paths)}
    return sorted(out, key=lambda r: order[r.path])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("paths", nargs="+", help=".smt2 files or directories")
    ap.add_argument("--budget", type=int, default=1 << 22, help="candidates per query")
    ap.add_argument("--batch", type=int, default=64, help="programs per launch")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--explain-misses", action="store_true",
                    help="profile every missed query: one line with its blocking conjuncts")
    ap.add_argument("--witness-density", action="store_true",
                    help="count every searched query's witnesses: one line with total / count and the first index")
    ap.add_argument("--repair-misses", action="store_true",
                    help="run WitnessEngine.repair on every missed query: one line with repaired or not, rounds, nfail")
    a = ap.parse_args(argv)
    files = []
    for p in a.paths:
        files += sorted(glob.glob(os.path.join(p, "*.smt2")) + glob.glob(os.path.join(p, "*.smt2.gz"))) \
            if os.path.isdir(p) else [p]
    from .engine import WitnessEngine
    eng = WitnessEngine(device=a.device, budget=a.budget)
    t0 = time.perf_counter()
    res = replay(files, eng, a.batch, explain=a.explain_misses, density=a.witness_density,
                 repair=REPAIR_ROUNDS if a.repair_misses else 0)
    dt = time.perf_counter() - t0
    for r in res:
        print(json.dumps({"file": os.path.basename(r.path), "status": r.status, "index": r.index,
                          "reason": r.reason}))
        if a.explain_misses and r.status == "miss":
            print(explain_line(r))
        if a.repair_misses and r.status == "miss":
            print(repair_line(r))
        if a.witness_density and r.status in ("witness", "miss"):
            print(density_line(r))
    summary = {k: sum(1 for r in res if r.status == k) for k in ("witness", "miss", "z3", "unsupported")}
    print(json.dumps({"files": len(res), **summary, "seconds": dt, "engine": eng.stats}), flush=True)
    eng.close()


if __name__ == "__main__":
    sys.exit(main())
