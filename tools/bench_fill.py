"""Time the row fill (sm_fill_invalid_device) at 1080p on device-resident maps:

  u8    the LR-checked, speckle-filtered AD-SGM map of the bench's synthetic pair (r = 2, D = 128, speckle 200 / 1);
  u16   the same from the sub-pixel call: the 1/16-px map.

The fill works in place, so every call is preceded by a device copy of the source map into the working map; the
hipEvents bracket the fill alone, one pair per call, and the figures are the median, the smallest and the largest
of `--iters` calls after `--warmup` calls.  In the same process, for scale: the 7 x 7 median (sm_median_u8_device)
on the uint8 map, the speckle filter (sm_speckle_filter_device) on the unfiltered LR-checked maps, and the whole
SGM call with the LR check, the fill off and on: match_device between hipEvents, and the host call match_lr by the
wall clock.  Two rounds over everything, so that a drift of the
machine shows as a spread.  Writes profiles/fill_bench.json, keeping a "headline" entry already there (the
alternated `python bench.py` runs of DESIGN §29 are recorded under it).  No GPU, no number: the script fails without one."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_speckle import per_call_ms  # noqa: E402

W, H, D, R = 1920, 1080, 128, 2
MAX_SIZE, RANGE = 200, 1
GAPS = (16, 1 << 24)      # a short limit, and every run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_bench.json"))
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    import torch
    import gpu_stereo_matching_amd as sm
    if not torch.cuda.is_available():
        raise SystemExit("bench_fill: no GPU visible; nothing is measured on a CPU")
    res = {"workload": {"width": W, "height": H, "num_disp": D, "radius": R, "pair": "synth_pair(1234)",
                        "speckle": [MAX_SIZE, RANGE], "max_gap": list(GAPS)},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters,
           "timing": "hipEvents around each call; the copy that restores the map is outside them",
           "workspace_bytes": 0, "runs": {}}
    runs = res["runs"]
    with sm.BlockMatcher(0, W, H, D) as m:
        L, Rr = sm.synth_pair(1234, W, H, D)
        Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(Rr).cuda()
        raw8 = m.match_device(Lt, Rt, R, D, agg="sgm", lr_check=True)
        raw16 = m.match_subpix_device(Lt, Rt, R, D, agg="sgm", lr_check=True)
        torch.cuda.synchronize()
        m8 = m.speckle_filter_device(raw8.clone(), MAX_SIZE, RANGE)
        m16 = m.speckle_filter_device(raw16.clone(), MAX_SIZE, 16 * RANGE)
        torch.cuda.synchronize()
        w8, w16 = torch.empty_like(m8), torch.empty_like(m16)
        med_out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        for rnd in range(2):
            for gap in GAPS:
                key = "all" if gap >= W else str(gap)
                runs.setdefault("fill_u8_gap_" + key, []).append(per_call_ms(
                    torch, lambda: w8.copy_(m8), lambda: m.fill_invalid_device(w8, gap), a.warmup, a.iters))
                runs["filled_pixels_u8_gap_" + key] = int(((m8 == 0) & (w8 != 0)).sum().item())
                runs.setdefault("fill_u16_gap_" + key, []).append(per_call_ms(
                    torch, lambda: w16.copy_(m16), lambda: m.fill_invalid_device(w16, gap), a.warmup, a.iters))
                runs["filled_pixels_u16_gap_" + key] = int(((m16 == 0) & (w16 != 0)).sum().item())
            runs.setdefault("median7x7_u8", []).append(per_call_ms(
                torch, lambda: None, lambda: m.median_device(m8, 3, out_t=med_out), a.warmup, a.iters))
            runs.setdefault("speckle_u8", []).append(per_call_ms(
                torch, lambda: w8.copy_(raw8), lambda: m.speckle_filter_device(w8, MAX_SIZE, RANGE), a.warmup,
                a.iters))
            runs.setdefault("speckle_u16", []).append(per_call_ms(
                torch, lambda: w16.copy_(raw16), lambda: m.speckle_filter_device(w16, MAX_SIZE, 16 * RANGE), a.warmup,
                a.iters))
            for gap, key in ((0, "fill_off"), (GAPS[-1], "fill_on")):
                m.set_fill(gap)
                try:
                    runs.setdefault("match_device_lr_sgm_" + key, []).append(per_call_ms(
                        torch, lambda: None,
                        lambda: m.match_device(Lt, Rt, R, D, out_t=out, agg="sgm", lr_check=True), a.warmup, a.iters))
                    # the host call (pageable frames up, three maps down): wall clock, it ends in a synchronise
                    ms = []
                    for k in range(a.warmup + a.iters):
                        t0 = time.perf_counter()
                        m.match_lr(L, Rr, R, D, agg="sgm")
                        ms.append((time.perf_counter() - t0) * 1e3)
                    ms = ms[a.warmup:]
                    runs.setdefault("match_lr_sgm_host_" + key, []).append(
                        {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                         "max_ms": round(max(ms), 4)})
                finally:
                    m.set_fill(0)
        runs["invalid_pixels_u8"] = int((m8 == 0).sum().item())
        runs["invalid_pixels_u16"] = int((m16 == 0).sum().item())
    if os.path.exists(a.out):   # the alternated bench.py runs, written down beside these times by hand
        kept = json.load(open(a.out)).get("headline")
        if kept:
            res["headline"] = kept
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
