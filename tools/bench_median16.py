"""Time the 16-bit median (sm_median_u16_device) at 1080p on a device-resident map:

  median16_r1 / _r2 / _r3   on the LR-checked 1/16-px AD-SGM map of the bench's synthetic pair (r = 2, D = 128);
  median7x7_u8              sm_median_u8_device at radius 3 on the 8-bit map of the same pair, the yardstick;
  match_subpix_lr_sgm_m0 / _m1 / _m3
                            the sub-pixel SGM call with the LR check, SM_PARAM_SUBPIX_MEDIAN at 0, 1 and 3.

hipEvents bracket each call, one pair per call, and the figures are the median, the smallest and the largest of
`--iters` calls after `--warmup` calls.  Two rounds over everything, alternated in one process, so that a drift of
the machine shows as a spread.  Writes profiles/median16_bench.json, keeping a "headline" entry already there (the
alternated `python bench.py` runs of DESIGN §33 are recorded under it).  No GPU, no number: the script fails
without one."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_speckle import per_call_ms  # noqa: E402

W, H, D, R = 1920, 1080, 128, 2
RADII = (1, 2, 3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median16_bench.json"))
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    import torch
    import gpu_stereo_matching_amd as sm
    if not torch.cuda.is_available():
        raise SystemExit("bench_median16: no GPU visible; nothing is measured on a CPU")
    res = {"workload": {"width": W, "height": H, "num_disp": D, "radius": R, "pair": "synth_pair(1234)",
                        "median_radii": list(RADII)},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters,
           "timing": "hipEvents around each call", "runs": {}}
    runs = res["runs"]
    with sm.BlockMatcher(0, W, H, D) as m:
        L, Rr = sm.synth_pair(1234, W, H, D)
        Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(Rr).cuda()
        m8 = m.match_device(Lt, Rt, R, D, agg="sgm", lr_check=True)
        m16 = m.match_subpix_device(Lt, Rt, R, D, agg="sgm", lr_check=True)
        torch.cuda.synchronize()
        out8, out16 = torch.empty_like(m8), torch.empty_like(m16)
        sub = torch.empty_like(m16)
        for rnd in range(2):
            for r in RADII:
                runs.setdefault(f"median16_r{r}", []).append(per_call_ms(
                    torch, lambda: None, lambda: m.median16_device(m16, r, out_t=out16), a.warmup, a.iters))
                runs[f"changed_pixels_r{r}"] = int((out16 != m16).sum().item())
            runs.setdefault("median7x7_u8", []).append(per_call_ms(
                torch, lambda: None, lambda: m.median_device(m8, 3, out_t=out8), a.warmup, a.iters))
            for r in (0, 1, 3):
                m.set_subpix_median(r)
                try:
                    runs.setdefault(f"match_subpix_lr_sgm_m{r}", []).append(per_call_ms(
                        torch, lambda: None,
                        lambda: m.match_subpix_device(Lt, Rt, R, D, out_t=sub, agg="sgm", lr_check=True), a.warmup,
                        a.iters))
                    runs[f"valid_pixels_m{r}"] = int((sub != 0).sum().item())
                finally:
                    m.set_subpix_median(0)
        runs["invalid_pixels_u16"] = int((m16 == 0).sum().item())
    med = lambda key: min(x["median_ms"] for x in runs[key])  # noqa: E731
    res["ratios"] = {f"median16_r{r}_over_median7x7_u8": round(med(f"median16_r{r}") / med("median7x7_u8"), 3)
                     for r in RADII}
    res["ratios"].update({f"median_m{r}_share_of_subpix_call": round(
        (med(f"match_subpix_lr_sgm_m{r}") - med("match_subpix_lr_sgm_m0")) / med("match_subpix_lr_sgm_m0"), 4)
        for r in (1, 3)})
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
