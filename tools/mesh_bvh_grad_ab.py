#!/usr/bin/env python3
"""The A/B record of the large-mesh gradient (profiles/mesh_bvh_grad_ab.json) and the parent's figures in profiles/mesh_bvh_grad_probe.json.

  python tools/mesh_bvh_grad_ab.py run LABEL DIR     in a tree with a built library (this commit's, or a checkout of its parent with this
                                                     file and tools/mesh_bvh_grad_probe.py copied in): tools/mesh_probe.py, tools/hull_probe.py
                                                     and `python bench.py --gpus 1 --steps 20 --warmup 3` once, into DIR/ab_LABEL_mesh.json,
                                                     DIR/ab_LABEL_hull.json, DIR/ab_LABEL_bench.jsonl.  LABEL: new_1, parent_1, new_2, parent_2,
                                                     in that order on one card.  With LABEL parent_1 also tools/mesh_bvh_grad_probe.py
                                                     --scale-only into DIR/parent_scale.json.
  python tools/mesh_bvh_grad_ab.py merge DIR         DIR/ab_* -> profiles/mesh_bvh_grad_ab.json; and, where DIR holds them,
                                                     DIR/mesh_bvh_grad_probe.json (this commit's tools/mesh_bvh_grad_probe.py --out) with
                                                     DIR/parent_scale.json as `for_scale_on_the_parent_commit` and the registers of the tree
                                                     kernels (tools/kernel_regs.py) as `kernels` -> profiles/mesh_bvh_grad_probe.json.

`summary` of the A/B record, per figure: the two runs of each side, the difference of the means, the parent's spread |run 1 - run 2|, and
`not_slower_beyond_parent_spread`: the new mean is at most the parent's mean + the parent's spread (a faster new side passes whatever
the spread)."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = ("new_1", "parent_1", "new_2", "parent_2")
TREE_KERNELS = ("fbr_mesh_bvh_grad_dist_kernel", "fbr_mesh_bvh_pairs_kernel", "fbr_mesh_grad_dist_kernel")


def run(label, out):
    os.makedirs(out, exist_ok=True)
    py = sys.executable
    subprocess.check_call([py, os.path.join(ROOT, "tools", "mesh_probe.py"), "--out", os.path.join(out, f"ab_{label}_mesh.json")], cwd=ROOT, stdout=subprocess.DEVNULL)
    subprocess.check_call([py, os.path.join(ROOT, "tools", "hull_probe.py"), "--out", os.path.join(out, f"ab_{label}_hull.json")], cwd=ROOT, stdout=subprocess.DEVNULL)
    line = subprocess.check_output([py, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=ROOT, text=True).strip().splitlines()[-1]
    with open(os.path.join(out, f"ab_{label}_bench.jsonl"), "w") as fh:
        fh.write(line + "\n")
    if label == "parent_1":
        subprocess.check_call([py, os.path.join(ROOT, "tools", "mesh_bvh_grad_probe.py"), "--scale-only", "--out", os.path.join(out, "parent_scale.json")],
                              cwd=ROOT, stdout=subprocess.DEVNULL)


def call_figures(d, pre=""):
    """{dotted name: ms} of the call times of a probe's record"""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(call_figures(v, pre + k + "."))
        elif k in ("call_ms", "convex", "mesh") and isinstance(v, (int, float)):
            out[pre + k] = float(v)
    return out


def merge(src):
    ab = {"what": "tools/mesh_probe.py, tools/hull_probe.py and python bench.py --gpus 1 --steps 20 --warmup 3 on this commit (new) and on its parent, "
                  "alternating new, parent, new, parent on one MI355X (tools/mesh_bvh_grad_ab.py); call_ms medians of 5 repetitions each"}
    flat = {}
    for label in LABELS:
        rec = {"mesh_probe": json.load(open(os.path.join(src, f"ab_{label}_mesh.json"))), "hull_probe": json.load(open(os.path.join(src, f"ab_{label}_hull.json")))}
        b = json.loads(open(os.path.join(src, f"ab_{label}_bench.jsonl")).read().strip().splitlines()[-1])
        rec["bench"] = {k: b[k] for k in ("value", "ms_per_step", "kernel_ms_per_step", "gram_checksum") if k in b}
        ab[label] = rec
        flat[label] = dict(call_figures({"mesh_probe": rec["mesh_probe"], "hull_probe": rec["hull_probe"]}), **{"bench.ms_per_step": float(b["ms_per_step"])})
    ab["summary"] = {"rule": "not_slower_beyond_parent_spread: mean(new) <= mean(parent) + |parent_1 - parent_2|"}
    for k in flat["new_1"]:
        p, n = [flat["parent_1"][k], flat["parent_2"][k]], [flat["new_1"][k], flat["new_2"][k]]
        spread, diff = abs(p[0] - p[1]), sum(n) / 2 - sum(p) / 2
        ab["summary"][k] = {"parent": p, "new": n, "difference_of_means": diff, "parent_spread": spread, "not_slower_beyond_parent_spread": bool(diff <= spread)}
    with open(os.path.join(ROOT, "profiles", "mesh_bvh_grad_ab.json"), "w") as fh:
        json.dump(ab, fh, indent=1)
    for k, v in ab["summary"].items():
        if k != "rule":
            print(f"{k}: parent {v['parent'][0]:.3f} / {v['parent'][1]:.3f}, new {v['new'][0]:.3f} / {v['new'][1]:.3f}, {v['not_slower_beyond_parent_spread']}")
    probe, scale = os.path.join(src, "mesh_bvh_grad_probe.json"), os.path.join(src, "parent_scale.json")
    if not (os.path.exists(probe) and os.path.exists(scale)):
        return
    d, ps = json.load(open(probe)), json.load(open(scale))
    for C in ("C16", "C64"):
        d[C]["for_scale_on_the_parent_commit"] = ps[C]["for_scale"]
    regs = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py")], text=True)
    d["kernels"] = {}
    for line in regs.splitlines():
        m = re.search(r"vgpr=\s*(\d+) agpr=\s*(\d+) vspill=\s*(\d+) sgpr=\s*(\d+) sspill=\s*(\d+) scratch=\s*(\d+) lds=\s*(\d+)\s+(\w+)", line)
        if m and m.group(8) in TREE_KERNELS:
            d["kernels"][m.group(8)] = dict(zip(("vgpr", "agpr", "vgpr_spill", "sgpr", "sgpr_spill", "scratch_bytes", "lds_bytes"), map(int, m.groups()[:7])))
    d["what"] = ("tools/mesh_bvh_grad_probe.py on one MI355X; for_scale_on_the_parent_commit: its --scale-only mode run from the parent commit's tree and "
                 "library in the same visit; kernels: tools/kernel_regs.py on this commit's library (merged by tools/mesh_bvh_grad_ab.py)")
    with open(os.path.join(ROOT, "profiles", "mesh_bvh_grad_probe.json"), "w") as fh:
        json.dump(d, fh, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "run" and sys.argv[2] in LABELS:
        run(sys.argv[2], os.path.abspath(sys.argv[3]))
    elif len(sys.argv) == 3 and sys.argv[1] == "merge":
        merge(os.path.abspath(sys.argv[2]))
    else:
        sys.exit(__doc__)
