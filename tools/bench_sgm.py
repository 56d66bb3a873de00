"""Time SM_AGG_SGM at 1080p, D = 128, r = 2 on the device-resident path (sm_match_device on torch tensors),
without and with the LR check: hipEvents around `--iters` calls after `--warmup` calls, frames already in HBM.
Writes profiles/sgm_bench.json: ms per frame, the algorithmic bytes of the design spelled out as a formula,
and that traffic over the time as a fraction of the 6.85 TB/s fill rate the project measured
(profiles/microbench/r05_write_ceiling.txt).  No GPU, no number: the script fails without one.

--paths 8 times the same two calls with the diagonal paths on (SM_PARAM_SGM_PATHS 8) and writes
profiles/sgm_bench_paths8.json; the default, 4, writes the files named here.

--pairs in-view [--min-disp N] times the same two calls under SM_PAIRS_IN_VIEW, with SM_PARAM_MIN_DISP N, and writes
profiles/sgm_bench_in_view.json; --disp stays the number of planes, so the search is N .. N + disp - 1.

--cost census times the census cost (SM_COST_CENSUS) under --agg sgm or box instead, beside AD SGM from the same run
of the same build, and writes profiles/census_bench.json (ms per map only: DESIGN §18).

--subpix times the sub-pixel call (sm_match_subpix_device, uint16 maps in 1/16 px) alternated with the 8-bit call of
the same flags, for AD SGM and census SGM without and with LR, with the uniqueness filter off and at 10, and writes
profiles/subpix_bench.json (ms per map and the difference: DESIGN §20)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILL_BYTES_PER_S = 6.85e12

# per frame, P = W * H pixels, D disparities (bytes); an atomic add counts its read and its write
FORMULA = {
    "ad_volume": "2*P + P*D            (read the pair, write the u8 AD volume)",
    "sad_volume": "P*D + 2*P*D          (read AD, write the u16 SAD volume)",
    "zero_S": "4*P*D                (memset of the u32 sum volume)",
    "paths_horizontal": "2 * (2*P*D + 8*P*D)  (per direction: read SAD u16, atomic-add S u32 = read + write)",
    "paths_vertical": "2 * (2*P*D + 8*P*D)  (the same)",
    "wta_left": "4*P*D + P            (read S, write the u8 map)",
    "wta_right_lr_only": "4*P*D + 4*P + 4*P + P + 3*P  (read S along u + d, write and read the keys, write dR; the check reads two maps, writes one)",
}


FORMULA_DIAGONAL = "4 * (2*P*D + 8*P*D)  (--paths 8: the same per direction, four diagonals)"


def algorithmic_bytes(P, D, lr, paths=4):
    b = (2 * P + P * D) + 3 * P * D + 4 * P * D + 2 * 10 * P * D + 2 * 10 * P * D + (4 * P * D + P)
    if paths == 8:
        b += 4 * 10 * P * D
    if lr:
        b += 4 * P * D + 4 * P + 4 * P + P + 3 * P
    return b


def time_ms(torch, m, Lt, Rt, r, D, out_t, warmup, iters, **kw):
    for _ in range(warmup):
        m.match_device(Lt, Rt, r, D, out_t=out_t, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        m.match_device(Lt, Rt, r, D, out_t=out_t, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def census_main(a, sm, torch, Lt, Rt, out_t):
    """ms per map of the census cost under a.agg, without and with LR, and of AD SGM in the same run."""
    W, H, D, r = a.width, a.height, a.disp, a.radius
    res = {"workload": {"width": W, "height": H, "num_disp": D, "radius": r, "cost": "census", "agg": a.agg,
                        "penalties": sm.sgm_penalties(r, cost="census") if a.agg == "sgm" else None},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters,
           "workspace_bytes": sm.census_workspace_bytes(W, H, D, r, agg=a.agg), "runs": {}}
    with sm.BlockMatcher(0, W, H, D) as m:
        # two rounds, alternating the variants, so that a drift of the machine shows as a spread
        for rnd in range(2):
            for name, kw in ((f"census_{a.agg}", dict(agg=a.agg, cost="census", lr_check=False)),
                             (f"census_{a.agg}_lr", dict(agg=a.agg, cost="census", lr_check=True)),
                             ("ad_sgm", dict(agg="sgm", lr_check=False)),
                             ("ad_sgm_lr", dict(agg="sgm", lr_check=True))):
                ms = time_ms(torch, m, Lt, Rt, r, D, out_t, a.warmup, a.iters, **kw)
                run = res["runs"].setdefault(name, {"ms_per_frame": []})
                run["ms_per_frame"].append(round(ms, 4))
                run["matched_pixels"] = int((out_t > 0).sum().item())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


def subpix_main(a, sm, torch, Lt, Rt, out_t):
    """ms per map of the sub-pixel call and of the 8-bit call of the same flags, alternated, two rounds."""
    W, H, D, r = a.width, a.height, a.disp, a.radius
    res = {"workload": {"width": W, "height": H, "num_disp": D, "radius": r, "agg": "sgm"},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "runs": {}}
    out16 = torch.empty((H, W), dtype=torch.int16, device=Lt.device)

    def time16(m, **kw):
        for _ in range(a.warmup):
            m.match_subpix_device(Lt, Rt, r, D, out_t=out16, **kw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            m.match_subpix_device(Lt, Rt, r, D, out_t=out16, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    with sm.BlockMatcher(0, W, H, D) as m:
        for rnd in range(2):
            for u in (0, 10):
                m.set_uniqueness(u)
                for cost in ("ad", "census"):
                    for lr in (False, True):
                        kw = dict(agg="sgm", cost=cost, lr_check=lr)
                        ms8 = time_ms(torch, m, Lt, Rt, r, D, out_t, a.warmup, a.iters, **kw)
                        ms16 = time16(m, **kw)
                        run = res["runs"].setdefault(f"{cost}_sgm{'_lr' if lr else ''}_u{u}",
                                                     {"ms_8bit": [], "ms_subpix": [], "ms_difference": []})
                        run["ms_8bit"].append(round(ms8, 4))
                        run["ms_subpix"].append(round(ms16, 4))
                        run["ms_difference"].append(round(ms16 - ms8, 4))
                        run["valid_pixels_subpix"] = int((out16 > 0).sum().item())
                        run["valid_pixels_8bit"] = int((out_t > 0).sum().item())
        m.set_uniqueness(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--disp", type=int, default=128)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--cost", default="ad", choices=["ad", "census"])
    ap.add_argument("--agg", default="sgm", choices=["sgm", "box"])
    ap.add_argument("--subpix", action="store_true", help="time the sub-pixel call against the 8-bit call (AD and census SGM)")
    ap.add_argument("--paths", type=int, default=4, choices=[4, 8],
                    help="scan directions of AD SGM (SM_PARAM_SGM_PATHS): 8 adds the diagonals and writes "
                         "profiles/sgm_bench_paths8.json")
    ap.add_argument("--pairs", default="reference", choices=["reference", "in-view"],
                    help="pair rule of AD SGM: in-view is SM_PAIRS_IN_VIEW and writes "
                         "profiles/sgm_bench_in_view.json")
    ap.add_argument("--min-disp", type=int, default=0, help="SM_PARAM_MIN_DISP, with --pairs in-view")
    ap.add_argument("--out", default=None,
                    help="default: profiles/sgm_bench.json, census_bench.json with --cost census, subpix_bench.json with --subpix")
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    if a.cost == "ad" and a.agg != "sgm":
        ap.error("--agg box is timed with --cost census only (the AD box path is bench.py's)")
    if a.paths == 8 and (a.subpix or a.cost != "ad"):
        ap.error("--paths 8 is timed on the AD SGM calls only")
    if a.pairs != "in-view" and a.min_disp:
        ap.error("--min-disp needs --pairs in-view")
    if a.pairs == "in-view" and (a.subpix or a.cost != "ad"):
        ap.error("--pairs in-view is timed on the AD SGM calls only")
    if a.out is None:
        name = "subpix_bench.json" if a.subpix else ("sgm_bench.json" if a.cost == "ad" else "census_bench.json")
        if a.paths == 8:
            name = "sgm_bench_paths8.json"
        if a.pairs == "in-view":
            name = "sgm_bench_in_view.json"
        a.out = os.path.join(ROOT, "profiles", name)
    import torch
    import gpu_stereo_matching_amd as sm
    if not torch.cuda.is_available():
        raise SystemExit("bench_sgm: no GPU visible; nothing is measured on a CPU")
    W, H, D, r = a.width, a.height, a.disp, a.radius
    P = W * H
    L, R = sm.synth_pair(1234, W, H, D)
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    out_t = torch.empty_like(Lt)
    if a.subpix:
        return subpix_main(a, sm, torch, Lt, Rt, out_t)
    if a.cost == "census":
        return census_main(a, sm, torch, Lt, Rt, out_t)
    res = {"workload": {"width": W, "height": H, "num_disp": D, "radius": r, "penalties": sm.sgm_penalties(r)},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters,
           "workspace_bytes": sm.sgm_workspace_bytes(W, H, D, r),
           "algorithmic_bytes_formula": FORMULA, "fill_rate_bytes_per_s": FILL_BYTES_PER_S, "runs": {}}
    if a.paths == 8:
        res["workload"]["paths"] = 8
        res["algorithmic_bytes_formula"] = dict(FORMULA, paths_diagonal=FORMULA_DIAGONAL)
    kw = {}
    if a.pairs == "in-view":   # (a build without the flag is timed without the keyword)
        res["workload"].update(pairs="in-view", min_disp=a.min_disp)
        kw["pairs"] = "in-view"
    with sm.BlockMatcher(0, W, H, D) as m:
        if a.paths != 4:
            m.set_sgm_paths(a.paths)
        if a.min_disp:
            m.set_min_disp(a.min_disp)
        for name, lr in (("sgm", False), ("sgm_lr", True)):
            for _ in range(a.warmup):
                m.match_device(Lt, Rt, r, D, out_t=out_t, agg="sgm", lr_check=lr, **kw)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                m.match_device(Lt, Rt, r, D, out_t=out_t, agg="sgm", lr_check=lr, **kw)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            nbytes = algorithmic_bytes(P, D, lr, a.paths)
            res["runs"][name] = {"ms_per_frame": round(ms, 4), "algorithmic_bytes": nbytes,
                                 "algorithmic_GB_per_s": round(nbytes / ms / 1e6, 1),
                                 "fraction_of_fill_rate": round(nbytes / (ms * 1e-3) / FILL_BYTES_PER_S, 4),
                                 "matched_pixels": int((out_t > 0).sum().item())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
