#!/usr/bin/env python3
"""The fused Gram over sample-contiguous images (option gram_lane, csrc/fbr_gram64.h) against the per-sample-image pass: time per call
(blocking and two submissions in flight; median of --runs runs with their spread), kernel split, agreement of the two Grams.

  --k 1,2     rhs columns of the calls (0: none), one set of figures per value
  --runs 7    timed runs per figure (a run: 5 blocking calls / 10 submissions)
  --robots walkman_apriori:1000000,walkman_apriori:125000,walkman_left_arm:500000,kuka_lwr4:500000"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_states  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
from flobaroid_amd.topology import Topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--k", default="1")
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--robots", default="walkman_apriori:1000000,walkman_apriori:125000,walkman_left_arm:500000,kuka_lwr4:500000")
args = ap.parse_args()
ks = [int(x) for x in args.k.split(",")]


def stats(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(float(np.min(ms)), 3), "max": round(float(np.max(ms)), 3)}


dev = torch.device("cuda", 0)
for spec in args.robots.split(","):
    robot, S = spec.split(":")[0], int(spec.split(":")[1])
    floating = robot != "kuka_lwr4"
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", robot + ".topology.json"))
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth_states(topo, S, 1, floating)[0].items()}
    for k in ks:
        res = {}
        Gs = {}
        for lane in (0, 1):
            eng = Engine(topo, floating=floating, options={"gram_lane": lane})
            eng.use_torch_stream()
            if lane:
                res["lane_info"] = eng.gram_lane_info(k, S)
                res["program_info"] = eng.gram_program_info(k, S)
            rhs = None
            if k:
                rhs = torch.randn((S * eng.rows, k), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
            G = eng.gram(st, rhs=rhs)
            Gs[lane] = G.clone()
            for _ in range(3):
                eng.gram(st, rhs=rhs, out=G)
            torch.cuda.synchronize()
            blocking = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                for _ in range(5):
                    eng.gram(st, rhs=rhs, out=G)
                torch.cuda.synchronize()
                blocking.append((time.perf_counter() - t0) / 5 * 1e3)
            eng.profile_enable(True)
            eng.profile_get()
            for _ in range(10):
                eng.gram(st, rhs=rhs, out=G)
            torch.cuda.synchronize()
            pr = eng.profile_get()
            eng.profile_enable(False)
            outs = [torch.zeros_like(G), torch.zeros_like(G)]
            eng.wait(eng.gram_submit(st, outs[0], rhs=rhs))
            torch.cuda.synchronize()
            piped = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                pend = None
                for i in range(10):
                    tk = eng.gram_submit(st, outs[i & 1], rhs=rhs)
                    if pend is not None:
                        eng.wait(pend)
                    pend = tk
                eng.wait(pend)
                torch.cuda.synchronize()
                piped.append((time.perf_counter() - t0) / 10 * 1e3)
            res[f"lane{lane}"] = {"blocking_ms": stats(blocking), "pipelined_ms": stats(piped),
                                  "kernel_ms": {c: round(v[0] / 10, 3) for c, v in pr.items() if v[1]},
                                  "repeat_bitwise": bool(torch.equal(outs[0], outs[1]) and torch.equal(outs[0], G))}
            eng.close()
        res["rel_diff_lane_vs_images"] = float(torch.linalg.norm(Gs[1] - Gs[0]) / torch.linalg.norm(Gs[0]))
        print(robot, S, "k", k, json.dumps(res), flush=True)
