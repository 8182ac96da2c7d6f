"""Decision-forest engines on one GPU: ``engine="native"`` (csrc/forest.hip) against
``engine="torch"`` in the same process, ``fit`` and ``predict_proba``.

Timing: hipEvents around each call, ``--warmup`` untimed calls, then the median of ``--runs``
timed ones with the spread (min .. max). One more native fit is instrumented per kernel family
and level (events around every ops.forest call; it is not part of the timed runs).

    python scripts/bench_forest.py --shape 0            # 1e6 x 32, 3 classes, 64 bins, 16 trees, depth 10
    python scripts/bench_forest.py --shape 1            # 1e7 x 100, 2 classes, 256 bins, 4 trees, depth 8
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harp_amd.models import trees as T  # noqa: E402
from harp_amd.ops import forest as F  # noqa: E402

SHAPES = [dict(n=10 ** 6, d=32, C=3, B=64, T=16, depth=10), dict(n=10 ** 7, d=100, C=2, B=256, T=4, depth=8)]


def make_data(n, d, C, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    s = X[:, 0] * 1.5 + X[:, d // 2] * X[:, d - 1].sign() + 0.4 * torch.randn(n, generator=g, device=dev)
    q = torch.quantile(s[:200000].double(), torch.linspace(0, 1, C + 1, dtype=torch.float64, device=dev)[1:-1])
    return X, torch.bucketize(s.double(), q)


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": runs}


def level_split(fit):
    """Per level and kernel family milliseconds of one native fit."""
    names = ["level_hist", "split_feature", "split_node", "route_count", "route_scatter", "feature_subset"]
    orig = {k: getattr(F, k) for k in names}
    marks = []

    def wrap(name):
        def f(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig[name](*a, **kw)
            e1.record()
            marks.append((name, e0, e1))
            return out
        return f

    for k in names:
        setattr(F, k, wrap(k))
    try:
        fit()
        torch.cuda.synchronize()
    finally:
        for k in names:
            setattr(F, k, orig[k])
    levels, cur = [], None
    for name, e0, e1 in marks:
        if name == "level_hist":
            cur = {}
            levels.append(cur)
        cur[name] = cur.get(name, 0.0) + e0.elapsed_time(e1)
    return levels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-runs", type=int, default=None, help="timed runs of the torch engine (default: --runs)")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sh = SHAPES[a.shape]
    dev = torch.device("cuda", 0)
    X, y = make_data(sh["n"], sh["d"], sh["C"], dev)
    th = T._bins(X, sh["B"])
    res = {"shape": sh, "device": torch.cuda.get_device_name(0)}

    def forest(engine):
        return T.DecisionForest(n_trees=sh["T"], max_depth=sh["depth"], n_bins=sh["B"], seed=1, engine=engine)

    fitted = {}

    def fit(engine):
        fitted[engine] = forest(engine).fit(X, y, num_classes=sh["C"], thresholds=th)

    engines = ["native"] + ([] if a.skip_torch else ["torch"])
    for engine in engines:
        runs = a.runs if engine == "native" or a.torch_runs is None else a.torch_runs
        try:
            res[engine + "_fit"] = timed(lambda: fit(engine), a.warmup, runs)
            res[engine + "_predict"] = timed(lambda: fitted[engine].predict_proba(X), a.warmup, runs)
            res[engine + "_train_acc"] = float((fitted[engine].predict(X) == y).double().mean())
        except torch.cuda.OutOfMemoryError as e:  # the torch engine's expanded [n, d, C] fp64 tensor
            res[engine + "_skipped"] = "out of memory: " + str(e).splitlines()[0]
            torch.cuda.empty_cache()
        print(json.dumps({k: v for k, v in res.items() if k.startswith(engine)}), flush=True)
    levels = level_split(lambda: fit("native"))
    res["native_levels_ms"] = levels
    res["native_tree_level_ms"] = [sum(l.values()) / sh["T"] for l in levels]
    res["atomic_floor_ms"] = sh["n"] * sh["d"] * sh["C"] * 8 / 1.3e12 * 1e3
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
