"""Time the guided cost volume and SM_AGG_GUIDED in the sub-pixel call at 1080p, D = 128, r = 5 on the
device-resident path (torch tensors already in HBM): hipEvents around `--iters` calls after `--warmup` calls.
Writes profiles/guided_subpix_bench.json:
  volume              sm_guided_volume_device, one launch for every d; its 4*P*D bytes of stores over the time as a
                      fraction of the 6.85 TB/s fill rate the project measured (profiles/microbench/r05_write_ceiling.txt)
  volume_by_slices    the same bytes by the route the library had before: D one-disparity sm_guided_slice_keys_device
                      calls (the d-independent guide statistics redone by each); ms per frame of all D
  subpix / subpix_lr  sm_match_subpix_device with agg guided, without and with the LR check
  guided8 / guided8_lr  the 8-bit guided map of sm_match_device, for comparison (no target)
Two rounds, the variants alternated, so that a drift of the machine shows as a spread.
--books adds the mean |d - gt| of the 8-bit and of the 1/16-px guided maps on Books (r = 2, D = 80, gt = disp1 / 3) over
the pixels with gt > 0 whose 8-bit disparity is within 1 of gt, as DESIGN §20 reports for SGM.
No GPU, no number: the script fails without one."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILL_BYTES_PER_S = 6.85e12


def timed(torch, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def books(sm, torch):
    golden = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(golden, "middlebury_gray.npz"))
    gt = np.load(os.path.join(golden, "middlebury_gt.npz"))["Books/disp1"].astype(np.float64) / 3.0
    L, R = g["Books/view1"], g["Books/view5"]
    r, D = 2, 80
    H, W = L.shape
    with sm.BlockMatcher(0, W, H, D) as m:
        m.set_guided_subpix(True)
        d8 = m.match(L, R, r, D, agg="guided").astype(np.float64)
        q = m.match_subpix(L, R, r, D, agg="guided").astype(np.float64) / 16.0
    sel = (gt > 0) & (np.abs(d8 - gt) <= 1)
    both = sel & (q > 0)
    return {"workload": {"scene": "Books", "width": W, "height": H, "radius": r, "num_disp": D},
            "pixels": int(sel.sum()), "pixels_valid_in_both": int(both.sum()),
            "mean_abs_error_8bit": round(float(np.abs(d8 - gt)[sel].mean()), 4),
            "mean_abs_error_subpix": round(float(np.abs(q - gt)[sel].mean()), 4),
            "mean_abs_error_8bit_valid_in_both": round(float(np.abs(d8 - gt)[both].mean()), 4),
            "mean_abs_error_subpix_valid_in_both": round(float(np.abs(q - gt)[both].mean()), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--disp", type=int, default=128)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--books", action="store_true", help="add the Books mean error of the 8-bit and 1/16-px maps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_subpix_bench.json"))
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    import torch
    import gpu_stereo_matching_amd as sm
    if not torch.cuda.is_available():
        raise SystemExit("bench_guided_subpix: no GPU visible; nothing is measured on a CPU")
    W, H, D, r = a.width, a.height, a.disp, a.radius
    P = W * H
    L, R = sm.synth_pair(1234, W, H, D)
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    out8 = torch.empty_like(Lt)
    out16 = torch.empty((H, W), dtype=torch.int16, device=Lt.device)
    vol = torch.empty((D, H, W), dtype=torch.int32, device=Lt.device)
    keys = torch.empty((H, W), dtype=torch.int32, device=Lt.device)
    res = {"workload": {"width": W, "height": H, "num_disp": D, "radius": r}, "device": torch.cuda.get_device_name(0),
           "warmup": a.warmup, "iters": a.iters, "workspace_bytes": sm.guided_workspace_bytes(W, H, D, r),
           "volume_store_bytes": 4 * P * D, "fill_rate_bytes_per_s": FILL_BYTES_PER_S, "runs": {}}
    with sm.BlockMatcher(0, W, H, D) as m:
        m.set_guided_subpix(True)

        def slices():
            for d in range(min(D, W + 1)):
                m.guided_slice_keys_device(Lt, Rt, r, d, d + 1, keys_t=keys)

        variants = (
            ("volume", lambda: m.guided_volume_device(Lt, Rt, r, D, out_t=vol)),
            ("volume_by_slices", slices),
            ("subpix", lambda: m.match_subpix_device(Lt, Rt, r, D, out_t=out16, agg="guided")),
            ("subpix_lr", lambda: m.match_subpix_device(Lt, Rt, r, D, out_t=out16, agg="guided", lr_check=True)),
            ("guided8", lambda: m.match_device(Lt, Rt, r, D, out_t=out8, agg="guided")),
            ("guided8_lr", lambda: m.match_device(Lt, Rt, r, D, out_t=out8, agg="guided", lr_check=True)),
        )
        for _ in range(2):
            for name, fn in variants:
                ms = timed(torch, fn, a.warmup, a.iters)
                res["runs"].setdefault(name, {"ms_per_frame": []})["ms_per_frame"].append(round(ms, 4))
        res["runs"]["subpix_lr"]["valid_pixels"] = int((out16 > 0).sum().item())
        res["runs"]["guided8_lr"]["valid_pixels"] = int((out8 > 0).sum().item())
    v = min(res["runs"]["volume"]["ms_per_frame"])
    s = min(res["runs"]["volume_by_slices"]["ms_per_frame"])
    res["runs"]["volume"]["store_GB_per_s"] = round(4 * P * D / v / 1e6, 1)
    res["runs"]["volume"]["fraction_of_fill_rate"] = round(4 * P * D / (v * 1e-3) / FILL_BYTES_PER_S, 4)
    res["runs"]["volume"]["speedup_over_slices"] = round(s / v, 2)
    if a.books:
        res["books"] = books(sm, torch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
