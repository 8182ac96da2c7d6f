"""Times dense naive Bayes train and predict, native engine against torch engine, on one GPU.

Device events around each call, WARMUP warm-ups, median of REPS; one JSON line per measurement
(stdout and ``--out``). ``gbps`` is the bytes of X over the time of ``ops.nb.class_sums`` alone
(label conversion, the one-pass kernel, the split reduce and the read of the error flag).

    python scripts/bench_nb.py [--n 2000000] [--out nb_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from harp_amd.models import naive_bayes as NB  # noqa: E402
from harp_amd.ops import nb as NBK  # noqa: E402

WARMUP, REPS = 2, 7


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[REPS // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nb.py needs a GPU")
    dev, C, n = torch.device("cuda", 0), a.classes, a.n
    lines = []
    for d in (256, 2048):
        for dtype in (torch.float32, torch.float64):
            g = torch.Generator(device=dev).manual_seed(d)
            X = torch.rand(n, d, device=dev, dtype=dtype, generator=g).mul_(8).floor_()
            y = torch.randint(0, C, (n,), device=dev, generator=g)
            model = NB.train(X, y, C, engine="native")
            differ = int((NB.predict(X, model, engine="native") != NB.predict(X, model)).sum())
            t_sums = timed(lambda: NBK.class_sums(X, y, C))
            rec = {"n": n, "d": d, "C": C, "dtype": str(dtype).split(".")[1], "class_sums_ms": t_sums,
                   "gbps": X.numel() * X.element_size() / t_sums / 1e6, "labels_differing_from_torch": differ}
            for engine in ("native", "torch"):
                rec[f"train_{engine}_ms"] = timed(lambda: NB.train(X, y, C, engine=engine))
                rec[f"predict_{engine}_ms"] = timed(lambda: NB.predict(X, model, engine=engine))
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            del X, y, model
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
