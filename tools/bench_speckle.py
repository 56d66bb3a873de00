"""Time the speckle filter (sm_speckle_filter_device) at 1080p on device-resident maps, uint8 and uint16 (1/16 px):

  sgm_lr   the LR-checked AD-SGM map of the bench's synthetic pair (r = 2, D = 128; uint16: the sub-pixel call's);
  equal    an all-equal map: one region of P pixels, the worst case of the count pass;
  random   random values without 0 and 255: (nearly) every pixel a region of its own.

The filter works in place, so every call is preceded by a device copy of the source map into the working map; the
hipEvents bracket the filter alone, one pair per call, and the figures are the median, the smallest and the largest
of `--iters` calls after `--warmup` calls.  In the same run the 7 x 7 median (sm_median_u8_device) is timed on the
same uint8 maps, for scale.  Writes profiles/speckle_bench.json.  No GPU, no number: the script fails without one.

--kernels MAP runs `rocprofv3 --kernel-trace --stats` (a run of its own per map, as a child process) on the uint8
map MAP and adds the per-kernel average times under "kernel_us" of that map's entry in the output file.
--drive MAP is that child: the filter alone, `--iters` times, on the uint8 map MAP."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, D, R = 1920, 1080, 128, 2
MAX_SIZE, RANGE = 200, 1
MAPS = ("sgm_lr", "equal", "random")


def make_maps(sm, torch, m, which=MAPS, u16=True):
    """{name: (uint8 tensor, int16 tensor holding uint16 bit patterns or None)}"""
    import numpy as np
    maps = {}
    if "sgm_lr" in which:
        L, Rr = sm.synth_pair(1234, W, H, D)
        Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(Rr).cuda()
        a = m.match_device(Lt, Rt, R, D, agg="sgm", lr_check=True)
        b = m.match_subpix_device(Lt, Rt, R, D, agg="sgm", lr_check=True) if u16 else None
        maps["sgm_lr"] = (a, b)
    if "equal" in which:
        maps["equal"] = (torch.full((H, W), 200, dtype=torch.uint8, device="cuda"),
                         torch.full((H, W), 3200, dtype=torch.int16, device="cuda") if u16 else None)
    if "random" in which:
        rng = np.random.default_rng(7)
        a = rng.integers(1, 255, (H, W)).astype(np.uint8)
        b = (a.astype(np.int16) * 16 + rng.integers(0, 16, (H, W)).astype(np.int16)) if u16 else None
        maps["random"] = (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda() if u16 else None)
    torch.cuda.synchronize()
    return maps


def per_call_ms(torch, prepare, call, warmup, iters):
    for _ in range(warmup):
        prepare()
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        prepare()
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def drive(a, sm, torch):
    with sm.BlockMatcher(0, W, H, D) as m:
        src = make_maps(sm, torch, m, (a.drive,), u16=False)[a.drive][0]
        work = torch.empty_like(src)
        for _ in range(a.iters):
            work.copy_(src)
            m.speckle_filter_device(work, MAX_SIZE, RANGE)
        torch.cuda.synchronize()
    return 0


def kernel_stats(a):
    out = tempfile.mkdtemp(prefix="speckle_kernels_" + a.kernels + "_")   # the trace is read below and not kept
    subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "k",
                    "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--drive", a.kernels,
                    "--iters", str(a.iters)], check=True, env=dict(os.environ, TMPDIR="/tmp"),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    us = {}
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "speckle" in row["Name"]:
                name = row["Name"].split("speckle_")[1].split("_kernel")[0]
                us[name] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) * 1e-3, 2)}
    if not us:
        raise SystemExit("bench_speckle: no speckle kernel in the trace")
    res = json.load(open(a.out)) if os.path.exists(a.out) else {"runs": {}}
    res["runs"].setdefault(a.kernels, {})["kernel_us"] = us
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({a.kernels: us}))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--kernels", choices=MAPS, default=None)
    ap.add_argument("--drive", choices=MAPS, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speckle_bench.json"))
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    if a.kernels:
        return kernel_stats(a)
    import torch
    import gpu_stereo_matching_amd as sm
    if not torch.cuda.is_available():
        raise SystemExit("bench_speckle: no GPU visible; nothing is measured on a CPU")
    if a.drive:
        return drive(a, sm, torch)
    res = {"workload": {"width": W, "height": H, "max_size": MAX_SIZE, "range": RANGE, "max_diff_u16": 16 * RANGE,
                        "sgm_lr_map": {"num_disp": D, "radius": R, "pair": "synth_pair(1234)"}},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters,
           "timing": "hipEvents around each call; the copy that restores the map is outside them",
           "workspace_bytes": sm.speckle_workspace_bytes(W, H), "runs": {}}
    with sm.BlockMatcher(0, W, H, D) as m:
        maps = make_maps(sm, torch, m)
        med_out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        for rnd in range(2):   # two rounds over the maps, so that a drift of the machine shows as a spread
            for name, (m8, m16) in maps.items():
                run = res["runs"].setdefault(name, {"u8": [], "u16": [], "median7x7_u8": []})
                w8, w16 = torch.empty_like(m8), torch.empty_like(m16)
                run["u8"].append(per_call_ms(torch, lambda: w8.copy_(m8),
                                             lambda: m.speckle_filter_device(w8, MAX_SIZE, RANGE), a.warmup, a.iters))
                run["u16"].append(per_call_ms(torch, lambda: w16.copy_(m16),
                                              lambda: m.speckle_filter_device(w16, MAX_SIZE, 16 * RANGE), a.warmup,
                                              a.iters))
                run["median7x7_u8"].append(per_call_ms(torch, lambda: None,
                                                       lambda: m.median_device(m8, 3, out_t=med_out), a.warmup, a.iters))
                run["valid_pixels_u8"] = int((m8 != 0).sum().item())
                run["removed_pixels_u8"] = int(((m8 != 0) & (w8 == 0)).sum().item())
                run["removed_pixels_u16"] = int(((m16 != 0) & (w16 == 0)).sum().item())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
