#!/usr/bin/env python3
"""Headline benchmark: disparity maps/s at 1080p, d_max=128 (BASELINE.json metric, cfg3).

A "step" is one pass of the hot path (fused AD + 11x11 box SAD + WTA, bit-exact with the
reference's getDisp / kernalFindCorr) over one batch of synthetic rectified 1920x1080 pairs
that are already resident in HBM when the timed region starts.

    python bench.py                      # N=1, defaults: the headline only
    python bench.py --full               # + CPU baselines, roofline, latency, cfg5, per-config table
    python bench.py --dump-outputs DIR   # + the last timed step's disparity maps as DIR/*.npy
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W [--full]

A plain run sets up, warms up, times exactly --steps steps and prints the result line.  Everything
else the benchmark measures or checks runs only with --full.

Multi-GPU: one process per GPU.  The path partitions by frame (independent pairs), so ranks
shard frames with no data-path collective ("scaling": "weak").  With --full, the two single-frame modes of
SURVEY §8e are measured in the same run for N > 1: "dslice" (cfg4: each rank owns a disparity
slice of the SAME 1080p d_max=256 frame; packed-key MIN reduce-scatter + uint8 all-gather over
RCCL, and the plain MIN all-reduce beside it) and "rowband" (each rank owns a band of rows plus an
r-row halo, all-gather of the uint8 bands).  "cfg5_guided_lr" (--full, every N) is BASELINE configs[4] as
written: 4K pairs, d_max=192, guided filter + LR check, frames batched over all ranks.

Rank 0 prints ONE JSON line.  Timing: barrier + synchronize on both sides of exactly K steps,
max over ranks.  With --full the dominant kernel's duration is measured live with HIP events on the
stream the kernels are launched on (torch's current stream, passed through the C ABI).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
# the fill ceiling measured on this part: torch's fill_ over 2.16 GB, one 16-B store per thread
# (profiles/microbench/r05_write_ceiling.txt): the best write stream seen, the reference for write-bound kernels
HBM_FILL_CEILING_GBS = 6850.0
# VALU issue peak: 256 CUs x 4 SIMDs, a wave64 VALU instruction issues over 2 cycles per SIMD (32 lanes
# per cycle, MI355X_MICROARCH.md "Execution model"), 2.4 GHz engine clock: 78.64 T lane-ops/s.  Measured
# on this part (profiles/microbench/r02_valu_issue_*.txt): add/sub/mul/fma/shift 2.4 cycles per
# wave-instruction, sad/perm/min/mul24/3-operand integer ops 4.2, cvt 7.7.
VALU_PEAK_TLANEOPS = 256 * 4 * 32 * 2.4e9 / 1e12
CU_CLOCK_HZ = 2.4e9


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--num-disp", type=int, default=128)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128,
                    help="frames per step per GPU (128 x 1080p pairs = 531 MB resident; amortises the launch tail: "
                         "18.2k maps/s vs 17.9k at 32 and 18.1k at 64, profiles/microbench/r02_headline_batch.txt)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: CPU baselines, per-step kernel events and the VALU roofline, batch-1 "
                         "latency, the N > 1 single-frame splits with their parity checks, cfg5 and the per-config table")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the disparity maps of the last step as DIR/<name>.npy (float32; "
                         "a fixed seeded sample of the pixels when the maps exceed the size budget)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-variants", action="store_true", help="with --full: skip the per-config / LR / guided table")
    ap.add_argument("--no-latency", action="store_true", help="with --full: skip the batch-1 latency measurement")
    ap.add_argument("--no-cfg5", action="store_true", help="with --full: skip the 4K guided+LR frame-parallel block")
    ap.add_argument("--profile", action="store_true",
                    help="--full without the CPU baselines, table, latency and cfg5: the timed steps with their kernel "
                         "events and roofline (what rocprof summaries under profiles/ are taken from)")
    ap.add_argument("--pmc-json", default=os.path.join(ROOT, "profiles", "pmc_box_r5_1080p.json"))
    ap.add_argument("--valu-json", default=os.path.join(ROOT, "profiles", "valu_counts.json"))
    return ap.parse_args()


def algorithmic_bytes_per_map(W: int, H: int, D: int) -> int:
    """the reference data flow moves B = P*(2D+3) bytes per map
    (L+R in, the D-plane uint8 AD volume written once and read once, disparity out)."""
    return W * H * (2 * D + 3)


def load_counts(path):
    try:
        with open(path) as f:
            return json.load(f).get("kernels", {})
    except (OSError, ValueError):
        return {}


def code_hash(symbol):
    """sha256 of the kernel's gfx950 machine code in the library this process loads (tools/codeobj.py)."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import codeobj
        from gpu_stereo_matching_amd import _capi
        return codeobj.kernel_sha256(_capi.LIB_PATH, symbol)
    except Exception as e:  # report, never hide
        return f"unavailable: {type(e).__name__}: {e}"


def valu_roofline(counts, key, workload, launch_ms, kernel, extra=None, symbol=None):
    """roofline on the binding resource of a compute-bound kernel: VALU lane-ops per second, from
    SQ_INSTS_VALU per launch (profiles/valu_counts.json, tools/valu_counts.py, same workload) over
    the live launch time; LDS-array busy fraction from SQ_LDS_IDX_ACTIVE beside it.  The counts are
    used only when their entry's code_sha256 is the hash of the machine code this process runs
    (VERDICT r5 item 3): after a kernel edit without a re-count, frac is null."""
    c = counts.get(key)
    if not c or c.get("workload") != list(workload):
        return {"bound": "valu", "achieved": None, "peak": round(VALU_PEAK_TLANEOPS, 2), "unit": "T lane-op/s",
                "frac": None, "kernel": kernel, "note": f"no SQ_INSTS_VALU count for {key} in profiles/valu_counts.json"}
    live = code_hash(symbol or c.get("code_symbol", ""))
    if c.get("code_sha256") != live:
        return {"bound": "valu", "achieved": None, "peak": round(VALU_PEAK_TLANEOPS, 2), "unit": "T lane-op/s",
                "frac": None, "kernel": kernel, "code_sha256": live, "counts_code_sha256": c.get("code_sha256"),
                "note": f"stale counts: profiles/valu_counts.json[{key}] was measured on other machine code than "
                        "the library loaded here; re-run tools/valu_counts.py"}
    pl = c["per_launch"]
    t = launch_ms * 1e-3
    achieved = pl["SQ_INSTS_VALU"] * 64 / t / 1e12
    res = {"bound": "valu", "achieved": round(achieved, 2), "peak": round(VALU_PEAK_TLANEOPS, 2),
           "unit": "T lane-op/s", "frac": round(achieved / VALU_PEAK_TLANEOPS, 4), "kernel": kernel,
           "kernel_ms_per_launch": round(launch_ms, 5), "valu_wave_insts_per_launch": pl["SQ_INSTS_VALU"],
           "lds_busy_frac": round(pl["SQ_LDS_IDX_ACTIVE"] / (256 * t * CU_CLOCK_HZ), 4)
           if "SQ_LDS_IDX_ACTIVE" in pl else None,
           "counts_source": "profiles/valu_counts.json (rocprofv3 --pmc SQ_INSTS_VALU, tools/valu_counts.py)",
           "code_sha256": live}
    # issue-cycle-weighted VALU busy: each wave64 VALU instruction costs the SIMD the cycles
    # measured for its encoding on this part (profiles/microbench/r02_valu_issue_cycles_pmc.txt: 2.37 for 32-bit
    # VOP1/VOP2, 4.25 for VOP3 such as v_perm_b32 / v_sad_u8 / v_min3_u32, 3.9 for conversions), averaged over
    # the kernel's unmasked main-loop iteration in the gfx950 ISA (profiles/isa_mix_box.json, tools/isa_mix.py);
    # SQ_INSTS_VALU x that average / (1024 SIMDs x launch cycles) is the share of the SIMDs' VALU issue
    # capacity the kernel uses with its own instruction mix
    try:
        with open(os.path.join(ROOT, "profiles", "isa_mix_box.json")) as f:
            mix = json.load(f)
    except (OSError, ValueError):
        mix = None
    if mix and key.startswith("box_r5") and mix.get("code_sha256") != live:
        res["valu_issue_busy"] = None
        res["valu_issue_note"] = "stale ISA mix: profiles/isa_mix_box.json describes other machine code"
    elif mix and key.startswith("box_r5"):
        cyc = pl["SQ_INSTS_VALU"] * mix["avg_cycles_per_valu"]
        res["valu_issue_busy"] = round(cyc / (1024 * t * CU_CLOCK_HZ), 4)
        res["valu_avg_cycles_per_inst"] = mix["avg_cycles_per_valu"]
        res["valu_issue_note"] = ("SQ_INSTS_VALU x measured issue cycles per instruction of the main-loop mix "
                                  f"({mix['valu_per_iteration']} VALU, {mix['issue_cycles_per_iteration']} cycles "
                                  "per wave and disparity pair) / SIMD cycles: the fraction of VALU issue capacity "
                                  "busy at this mix")
    W_, H_, D_, _r, B_ = workload
    res["lane_ops_per_pixel_d"] = round(pl["SQ_INSTS_VALU"] * 64 / (W_ * H_ * D_ * B_), 3)
    if "SQ_WAVE_CYCLES" in pl:
        res["wave_cycle_shares"] = {"issuing": round(pl["share_active_inst_any"], 4),
                                    "waiting_waitcnt_barrier": round(pl["share_wait_any"], 4),
                                    "issue_stalled": round(pl["share_wait_inst_any"], 4)}
    if extra:
        res.update(extra)
    return res


DUMP_BUDGET_BYTES = 64 << 20      # all files of one --dump-outputs run together
DUMP_SAMPLE_SEED = 20240531


def synth_batch(sm, seed0, n, W, H, D):
    """n synthetic pairs, seeds seed0 .. seed0 + n - 1, stacked to two [n, H, W] uint8 arrays; generated on
    the host cores this job may use (numpy releases the GIL), identical to calling synth_pair in a loop."""
    from concurrent.futures import ThreadPoolExecutor
    workers = max(1, min(16, n, len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(workers) as pool:
        pairs = list(pool.map(lambda i: sm.synth_pair(seed0 + i, W, H, D), range(n)))
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def dump_outputs(torch, directory, out, rank, world):
    """The maps the last timed step left in `out` ([B, H, W] uint8, what match_device hands its caller), as
    float32 .npy.  Each rank writes its own frames; the ranks share DUMP_BUDGET_BYTES.  A batch over the budget is
    written as the values at a fixed set of flat pixel indices (seeded, the same in every run and every build)."""
    os.makedirs(directory, exist_ok=True)
    name = "disparity" if world == 1 else f"disparity_rank{rank}"
    budget = DUMP_BUDGET_BYTES // world // 4 - 64        # float32 elements; 64 elements spare for the .npy header
    flat = out.reshape(-1)
    if flat.numel() > budget:
        # half the budget: enough pixels to see any frame or tile go wrong, and a small copy and file
        idx = np.random.default_rng(DUMP_SAMPLE_SEED).integers(0, flat.numel(), size=budget // 2, dtype=np.int64)
        flat = flat[torch.from_numpy(idx).to(out.device)]
        arr = flat.to(torch.float32).cpu().numpy()
    else:
        arr = flat.to(torch.float32).cpu().numpy().reshape(tuple(out.shape))
    np.save(os.path.join(directory, name + ".npy"), arr)


def cpu_baseline(W, H, D, r, seed):
    """Time the reference algorithm as written (getDisp restatement, early exit kept,
    gcc -O2, one thread) on one frame of the same synthetic workload."""
    from oracle import oracle as O
    O.build()
    L, R = O.synth_pair(seed, W, H, D)
    t0 = time.perf_counter()
    O.get_disp(L, R, r, D)
    dt = time.perf_counter() - t0
    return {"value": round(1.0 / dt, 5), "unit": "disparity-maps/s", "cores": 1, "kind": "port",
            "sample": f"1 frame {W}x{H} D={D} r={r} seed {seed}: oracle/bm_oracle.c ora_get_disp "
                      f"(restates BlockMatching.cpp:111-189 incl. early exit), gcc -O2, 1 thread, "
                      f"{dt:.2f} s/map"}


# BASELINE.json configs measured next to the headline (rank 0, device-resident pairs, `batch` frames per
# call).  cfg1/cfg2 run on the reference's bundled Middlebury pairs (their gray fixtures, committed under
# tests/golden); every other line uses synthetic pairs of the named size.
VARIANTS = (
    # name, W, H, D, r, agg, lr, median, batch
    # cfg1 / cfg2 on the reference's own bundled Middlebury pairs (Art, Books, Dolls; gray fixtures
    # in tests/golden, 463x370 — BASELINE's "450x375"), cycled to 96 frames per launch (9216 tiles, 9 rounds)
    ("cfg1 Middlebury Art/Books/Dolls 463x370 7x7 box d64", 463, 370, 64, 3, "box", False, False, 96),
    ("cfg2 Middlebury Art/Books/Dolls 463x370 9x9 box d64", 463, 370, 64, 4, "box", False, False, 96),
    # 1080p variants run 32 frames per launch, 4K 8 (the same ~38 rounds of
    # workgroups per launch): 4-frame launches lose 12-14 % to each launch's ramp-down
    ("cfg3 1080p 11x11 box+lr d128", 1920, 1080, 128, 5, "box", True, False, 32),
    ("cfg3 1080p 11x11 box+median7+lr d128", 1920, 1080, 128, 5, "box", True, True, 32),
    ("cfg3 1080p 11x11 guided d128", 1920, 1080, 128, 5, "guided", False, False, 32),
    ("cfg3 1080p 11x11 guided+lr d128", 1920, 1080, 128, 5, "guided", True, False, 32),
    ("cfg4 1080p 11x11 box d256", 1920, 1080, 256, 5, "box", False, False, 32),
    # wide windows (the reference's SADWindowSize is unbounded, Device.cu:46-56): r 8..15 on the fused kernel,
    ("1080p 17x17 box d128", 1920, 1080, 128, 8, "box", False, False, 32),
    ("1080p 23x23 box d128", 1920, 1080, 128, 11, "box", False, False, 32),
    ("1080p 31x31 box d128", 1920, 1080, 128, 15, "box", False, False, 32),
    ("1080p 31x31 box+lr d128", 1920, 1080, 128, 15, "box", True, False, 32),
    # r 16..37: the strip kernel (csrc/bm_strip.hip); r 38..127 the separable wide-window path
    # (csrc/bm_wide.hip)
    ("1080p 41x41 box d128", 1920, 1080, 128, 20, "box", False, False, 8),
    ("1080p 41x41 box+lr d128", 1920, 1080, 128, 20, "box", True, False, 8),
    ("1080p 255x255 box+lr d128", 1920, 1080, 128, 127, "box", True, False, 8),
    ("cfg5 4K 11x11 box d192", 3840, 2160, 192, 5, "box", False, False, 8),
    ("cfg5 4K 11x11 box+lr d192", 3840, 2160, 192, 5, "box", True, False, 8),
    ("cfg5 4K 11x11 guided+lr d192", 3840, 2160, 192, 5, "guided", True, False, 8),
)


def run_variants(sm, torch, dev, stream, seed):
    out = {}
    m = sm.BlockMatcher(dev.index, 3840, 2160, 256)
    try:
        frames = {}   # (W, H, D, B) -> device batch, shared by the variants of one shape
        for (name, W, H, D, r, agg, lr, med, B) in VARIANTS:
            try:
                if (W, H, D, B) not in frames:
                    frames.clear()
                    if name.startswith(("cfg1 Middlebury", "cfg2 Middlebury")):
                        g = np.load(os.path.join(ROOT, "tests", "golden", "middlebury_gray.npz"))
                        scenes = ("Art", "Books", "Dolls")
                        pairs = [(g[f"{scenes[i % 3]}/view1"], g[f"{scenes[i % 3]}/view5"]) for i in range(B)]
                    else:
                        pairs = [sm.synth_pair(seed + i, W, H, D) for i in range(B)]
                    frames[(W, H, D, B)] = (torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev),
                                            torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev))
                Lt, Rt = frames[(W, H, D, B)]
                o = torch.empty_like(Lt)
                for _ in range(2):
                    m.match_device(Lt, Rt, r, D, out_t=o, agg=agg, lr_check=lr, median=med, stream=stream)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                nrep = 10 if agg == "box" else 3
                e0.record(stream)
                for _ in range(nrep):
                    m.match_device(Lt, Rt, r, D, out_t=o, agg=agg, lr_check=lr, median=med, stream=stream)
                e1.record(stream)
                torch.cuda.synchronize(dev)
                ms = e0.elapsed_time(e1) / (nrep * B)
                out[name] = {"ms_per_frame": round(ms, 4), "maps_per_s": round(1000.0 / ms, 1), "frames_per_call": B}
            except Exception as e:  # report, never hide
                out[name] = {"error": str(e)}
        # row a1 on its own: the AD volume (PreCal / kernalPreCal_V2), an HBM-write-bound kernel
        W, H, D = 1920, 1080, 128
        L, R = sm.synth_pair(seed, W, H, D)
        Lt, Rt = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
        vol = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
        for _ in range(3):
            m.ad_volume_device(Lt, Rt, D, out_t=vol, stream=stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(20):
            m.ad_volume_device(Lt, Rt, D, out_t=vol, stream=stream)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1) / 20
        gbs = W * H * (D + 2) / (ms * 1e-3) / 1e9
        out["a1 AD volume 1080p d128 (PreCal, HBM-write-bound)"] = {
            "ms_per_frame": round(ms, 4), "achieved_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3),
            "bytes_per_frame": W * H * (D + 2)}
        del vol
        # the reference's two-kernel data flow through HBM volumes (SM_STAGED: AD u8 -> SAD u16 -> WTA),
        # bit-exact with the fused kernel; every byte of the three volumes crosses HBM.  8 frames per
        # call = one launch group (8 x 0.8 GB of volumes), as the fused path batches its frames
        SB = 8
        pairs = [sm.synth_pair(seed + i, W, H, D) for i in range(SB)]
        Ls = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
        Rs = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
        del pairs
        o1 = torch.empty_like(Ls)
        for _ in range(2):
            m.match_device(Ls, Rs, 5, D, out_t=o1, agg="box-staged", stream=stream)
        e0.record(stream)
        for _ in range(5):
            m.match_device(Ls, Rs, 5, D, out_t=o1, agg="box-staged", stream=stream)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1) / (5 * SB)
        nbytes = W * H * (D + 2) + 3 * W * H * D + (2 * W * H * D + W * H)
        gbs = nbytes / (ms * 1e-3) / 1e9
        out["staged box 1080p 11x11 d128 (AD u8 -> SAD u16 -> WTA through HBM, HBM-bound)"] = {
            "ms_per_frame": round(ms, 4), "maps_per_s": round(1000.0 / ms, 1), "achieved_GBs": round(gbs, 1),
            "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3), "bytes_per_frame": nbytes, "frames_per_call": SB}
        # per kernel: HIP events around each kernel launch of the 8-frame group (sm_last_staged_kernel_ms,
        # per frame), median of 10
        P = W * H
        per = {}
        kt = []
        for _ in range(10):
            m.match_device(Ls, Rs, 5, D, out_t=o1, agg="box-staged", stream=stream)
            kt.append(m.staged_kernel_ms())
        del Ls, Rs, o1
        kt = np.median(np.array(kt), axis=0)
        for kname, kms, nb in (("ad_volume_kernel", float(kt[0]), P * (D + 2)),
                               ("box_sad_kernel", float(kt[1]), 3 * P * D),
                               ("volume_wta_kernel", float(kt[2]), 2 * P * D + P)):
            g_ = nb / (kms * 1e-3) / 1e9
            per[kname] = {"ms": round(kms, 4), "algorithmic_bytes": nb, "achieved_GBs": round(g_, 1),
                          "frac_of_hbm_peak": round(g_ / HBM_PEAK_GBS, 3),
                          "frac_of_fill_ceiling": round(g_ / HBM_FILL_CEILING_GBS, 3), "frames_per_launch": SB}
        per["note"] = ("ms: HIP events around each kernel's launch on the product stream (median of 10 calls), so the "
                       "dispatch gap is inside it; rocprofv3's kernel durations (profiles/*staged_roofline*.json) time "
                       "the kernel alone and read 2-4 % higher fractions. The kernel's own roofline figure is the "
                       "rocprof one; these live figures bound it from below. frac_of_fill_ceiling: against "
                       f"{HBM_FILL_CEILING_GBS:.0f} GB/s, the fill rate measured on this part "
                       "(profiles/microbench/r05_write_ceiling.txt)")
        out["staged kernels 1080p d128 (HBM roofline per kernel)"] = per
        # host frame stream, PCIe-inclusive: FrameStream overlaps H2D / match / D2H on three streams;
        # frames are produced in place in the pinned slots (next_inputs) and consumed in place
        # (callback), so no host-side copy is timed
        from gpu_stereo_matching_amd.pipeline import FrameStream
        W, H, D, r, B = 1920, 1080, 128, 5, 8
        pairs = [sm.synth_pair(seed + i, W, H, D) for i in range(B)]
        Ls, Rs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        fs = FrameStream(m, B, W, H, r, D, consume=lambda disp: None)
        for k in range(fs.NS):                    # touch every pinned slot once before timing
            lv, rv = fs.next_inputs()
            lv[...] = Ls
            rv[...] = Rs
            fs.submit()
        fs.flush()
        nb = 48
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for k in range(nb):
            fs.next_inputs()                      # a producer would write the frames here
            fs.submit()
        fs.flush()
        ms = (time.perf_counter() - t0) * 1000 / (nb * B)
        out["host stream 1080p 11x11 box d128 (8-frame batches, pinned, overlapped)"] = {
            "ms_per_frame": round(ms, 4), "maps_per_s": round(1000.0 / ms, 1), "frames_per_call": B}
        # the drop-in host path (sm_block_match_u8: pageable H2D, match, D2H), PCIe-inclusive
        for (name, W, H, D, r) in (("host round trip 1080p 11x11 box d128", 1920, 1080, 128, 5),
                                   ("host round trip 463x370 9x9 box d64", 463, 370, 64, 4)):
            L, R = sm.synth_pair(seed, W, H, D)
            n = 20

            def timed(call):
                """ms per call of `call` with the handle at its default stage timing (auto, unarmed: no
                stage-split events), then the (upload, match, download) split of a few recorded calls"""
                m.set_stage_timing("auto")
                for _ in range(3):
                    call()
                t0 = time.perf_counter()
                for _ in range(n):
                    call()
                ms = (time.perf_counter() - t0) * 1000 / n
                m.stage_ms()                      # arms the recording for the calls below
                for _ in range(3):
                    call()
                up, mt, dn = m.stage_ms()
                m.set_stage_timing("auto")
                return ms, {"upload": round(up, 4), "match": round(mt, 4), "download": round(dn, 4)}

            ms, st = timed(lambda: m.match(L, R, r, D))
            out[name] = {"ms_per_frame": round(ms, 4), "maps_per_s": round(1000.0 / ms, 1), "frames_per_call": 1,
                         "stage_ms": st}
            # the same call on caller frames / map in sm_host_alloc (page-locked) memory
            Lp, Rp, Op = sm.host_empty((H, W)), sm.host_empty((H, W)), sm.host_empty((H, W))
            Lp[...] = L
            Rp[...] = R
            ms, st = timed(lambda: m.match(Lp, Rp, r, D, out=Op))
            out[name + " (sm_host_alloc buffers)"] = {
                "ms_per_frame": round(ms, 4), "maps_per_s": round(1000.0 / ms, 1), "frames_per_call": 1,
                "stage_ms": st}
            # the pair in one page-locked block (right frame after the left one): one upload copy
            pair = sm.host_empty((2, H, W))
            pair[0], pair[1] = L, R
            ms, st = timed(lambda: m.match(pair[0], pair[1], r, D, out=Op))
            out[name + " (sm_host_alloc, pair in one block)"] = {
                "ms_per_frame": round(ms, 4), "maps_per_s": round(1000.0 / ms, 1), "frames_per_call": 1,
                "stage_ms": st, "note": "timed at the default stage timing (no stage-split events); stage_ms "
                "from 3 recorded calls after the timed ones"}
            # the same with the stage-split events recorded in every call (SM_PARAM_STAGE_TIMING 1)
            m.set_stage_timing(True)
            for _ in range(3):
                m.match(pair[0], pair[1], r, D, out=Op)
            t0 = time.perf_counter()
            for _ in range(n):
                m.match(pair[0], pair[1], r, D, out=Op)
            ms = (time.perf_counter() - t0) * 1000 / n
            m.set_stage_timing("auto")
            out[name + " (sm_host_alloc, pair in one block, stage events in every call)"] = {
                "ms_per_frame": round(ms, 4), "maps_per_s": round(1000.0 / ms, 1), "frames_per_call": 1}
            del Lp, Rp, Op, pair
        # STMatching's segment-tree stereo, ST-1 and ST-2 (§8f rank 4), on the bundled Art pair at the app's
        # defaults: a synchronous host call (host segment_graph passes + GPU BFS / cost / filter / WTA / median /
        # LR check), wall
        g = np.load(os.path.join(ROOT, "tests", "golden", "middlebury_bgr.npz"))
        Lb, Rb = g["Art/view1"], g["Art/view5"]
        for method, label in ((0, "segment tree ST-1 Art 463x370 d60 (host segmentation + GPU BFS and filter, wall)"),
                              (1, "segment tree ST-2 Art 463x370 d60 (3 trees: host segmentation + GPU BFS, filters, LR check, wall)")):
            for _ in range(2):
                m.segment_tree(Lb, Rb, method=method)
            ts = []
            for _ in range(7):
                t0 = time.perf_counter()
                m.segment_tree(Lb, Rb, method=method)
                ts.append((time.perf_counter() - t0) * 1000)
            tree_ms, _, levels = m.segment_tree_stats()
            ms = float(np.median(ts))
            out[label] = {"ms_per_frame": round(ms, 3), "maps_per_s": round(1000.0 / ms, 1), "frames_per_call": 1,
                          "tree_ms": round(tree_ms, 3), "tree_levels": levels}
    finally:
        m.close()
    return out


def _cpu_one_frame(job):
    W, H, D, r, seed = job
    from oracle import oracle as O
    L, R = O.synth_pair(seed, W, H, D)
    O.get_disp(L, R, r, D)
    return 1


def cpu_baseline_all_cores(W, H, D, r, seed):
    """the same port on every host core this job may use (capped at 16, the GPU
    box's CPU share), one frame per process, reported as aggregate maps/s.  Runs before the
    GPU is initialised, so the forked workers inherit no device state."""
    import multiprocessing as mp
    from oracle import oracle as O
    O.build()
    n = max(1, min(16, len(os.sched_getaffinity(0))))
    ctx = mp.get_context("fork")
    with ctx.Pool(n) as pool:
        t0 = time.perf_counter()
        done = sum(pool.map(_cpu_one_frame, [(W, H, D, r, seed + i) for i in range(n)]))
        dt = time.perf_counter() - t0
    return {"value": round(done / dt, 4), "unit": "disparity-maps/s", "cores": n, "kind": "port",
            "sample": f"{n} frames {W}x{H} D={D} r={r}, one per process on {n} cores, {dt:.2f} s"}


def rank_inventory(torch, dist, dev, backend):
    """Every rank's device and PCI bus id (the first SCALE run records which GPUs it ran on)."""
    p = torch.cuda.get_device_properties(dev)
    bus = (getattr(p, "pci_domain_id", None), getattr(p, "pci_bus_id", None), getattr(p, "pci_device_id", None))
    mine = {"rank": dist.get_rank(), "device": dev.index, "name": p.name,
            "pci": "%04x:%02x:%02x" % bus if None not in bus else None}
    allr = [None] * dist.get_world_size()
    dist.all_gather_object(allr, mine)
    return {"backend": backend, "world": dist.get_world_size(), "ranks": allr}


def split_parity_box(sm, torch, dist, m, Lc, Rc, r, D4, rank, world, dev, stream):
    """Before any split is timed: one cfg4 frame d-sharded over the ranks, both collectives,
    against rank 0's single-GPU pass of the same frame, bit for bit on every rank (rank 0's map is broadcast and
    each rank compares its gathered copy; the mismatch count is MAX-reduced)."""
    from gpu_stereo_matching_amd import sharding
    H, W = Lc.shape
    ref = torch.empty((H, W), dtype=torch.uint8, device=dev)
    if rank == 0:
        m.match_device(Lc, Rc, r, D4, out_t=ref, stream=stream)
        torch.cuda.synchronize(dev)
    dist.broadcast(ref, 0)
    res = {}
    for coll in ("rs_ag", "allreduce"):
        got = sharding.match_dslice(m, Lc, Rc, r, D4, rank, world, stream=stream, collective=coll)
        torch.cuda.synchronize(dev)
        bad = torch.tensor([float((got != ref).sum().item())], dtype=torch.float64, device=dev)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        res[coll] = int(bad.item())
    return {"parity": all(v == 0 for v in res.values()), "rule": "bit-exact vs rank 0's single-GPU map, every rank",
            "mismatching_pixels_max_over_ranks": res}


def split_parity_guided_lr(sm, torch, dist, m5, L, R, r, D5, rank, world, dev, stream):
    """One cfg5 guided + LR frame d-sharded over the ranks (MIN all-reduce of the left and right slice keys, so
    every rank holds the reduced keys), against rank 0's single-member pass over [0, D5) of the same frame.
    Tie-aware equality: every pixel's reduced key has the single pass's cost field (the keys quantise q to 2^-14,
    and a slice's MIN picks the smallest quantised cost, so the cost fields must agree exactly); the d fields may
    differ only where two disparities tie on that cost; and every pixel where the checked maps differ has such a
    tie at its left pixel or at the right pixel either map points it to."""
    from gpu_stereo_matching_amd import sharding
    H, W = L.shape
    P = H * W
    kb = sharding.dslice_buffers(H, W, world, dev)
    rb = sharding.dslice_buffers(H, W, world, dev)
    chk = sharding.match_dslice(m5, L, R, r, D5, rank, world, keys_t=kb[0], out_t=kb[1], stream=stream,
                                agg="guided", lr_check=True, right_bufs=rb, collective="allreduce")
    torch.cuda.synchronize(dev)
    if rank != 0:
        dist.barrier()
        return None
    lk_ds, rk_ds = kb[0][:P].view(H, W).clone(), rb[0][:P].view(H, W).clone()
    chk_ds = chk.clone()
    lk, rk = m5.slice_keys_lr_device(L, R, r, 0, D5, agg="guided", stream=stream)
    left = m5.guided_keys_to_disp_device(lk)
    right = m5.right_keys_to_disp_device(rk)
    chk_1 = m5.lr_check_device(left, right)
    left_ds = m5.guided_keys_to_disp_device(lk_ds)
    fused = m5.match_device(L, R, r, D5, agg="guided", lr_check=True, stream=stream)
    torch.cuda.synchronize(dev)
    cost_l = bool(torch.equal(lk_ds >> 8, lk >> 8))
    cost_r = bool(torch.equal(rk_ds >> 8, rk >> 8))
    tie_l, tie_r = lk_ds != lk, rk_ds != rk
    xs = torch.arange(W, device=dev).view(1, W).expand(H, W)

    def right_tie_at(d):
        u = xs - d.long()
        return tie_r.gather(1, u.clamp(min=0)) & (u >= 0)

    mism = chk_ds != chk_1
    just = tie_l | right_tie_at(left_ds) | right_tie_at(left)
    unjust = int((mism & ~just).sum().item())
    dist.barrier()
    return {"parity": cost_l and cost_r and unjust == 0,
            "rule": "tie-aware: reduced key cost fields == single pass's (left and right), checked-map differences "
                    "only at cost ties",
            "left_cost_fields_equal": cost_l, "right_cost_fields_equal": cost_r,
            "left_d_ties": int(tie_l.sum().item()), "right_d_ties": int(tie_r.sum().item()),
            "checked_mismatch": int(mism.sum().item()), "checked_mismatch_unjustified": unjust,
            "checked_agreement_vs_fused_single_gpu_pass": round(float((chk_ds == fused).float().mean().item()), 6)}


def run_split_extras(sm, torch, dist, m, Lc, Rc, W, H, D, r, rank, world, dev, stream, backend, steps):
    """N > 1 only: one frame split over the ranks, d-slices (cfg4, d_max 256, MIN reduction of the slice keys,
    both collectives) and row bands (r-row halo, all-gather of uint8 bands); whole-job maps/s on the
    max-over-ranks clock.  Lc / Rc: the SAME frame on every rank (seeded alike), checked against rank 0's
    single-GPU map before the split is timed."""
    from gpu_stereo_matching_amd import sharding
    D4 = 256
    keys, dflat = sharding.dslice_buffers(H, W, world, dev)
    d1 = torch.empty((H, W), dtype=torch.uint8, device=dev)
    n = max(10, steps // 4)
    dslice = {"config": f"cfg4: {W}x{H} d_max={D4} r={r}, one frame d-sharded over {world} ranks",
              "unit": "disparity-maps/s", "scaling": "strong", "keys_bytes_per_frame": W * H * 4}
    dslice["check"] = split_parity_box(sm, torch, dist, m, Lc, Rc, r, D4, rank, world, dev, stream)
    for coll, label in (("rs_ag", f"reduce_scatter MIN int32 + all_gather uint8 ({backend})"),
                        ("allreduce", f"all_reduce MIN int32 ({backend})")):
        def dstep():
            sharding.match_dslice(m, Lc, Rc, r, D4, rank, world, keys_t=keys, out_t=dflat, stream=stream,
                                  collective=coll)

        for _ in range(5):
            dstep()
        torch.cuda.synchronize(dev)
        dist.barrier()
        t1 = time.perf_counter()
        for _ in range(n):
            dstep()
        torch.cuda.synchronize(dev)
        dist.barrier()
        dt = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        dslice[coll] = {"value": round(n / float(dt.item()), 2), "ms_per_frame": round(float(dt.item()) * 1000 / n, 4),
                        "collective": label}

    # row bands of one frame (r-row halo, all-gather of uint8 bands)
    # row bands: the same frame, checked like the d-slice before timing
    ref = torch.empty((H, W), dtype=torch.uint8, device=dev)
    if rank == 0:
        m.match_device(Lc, Rc, r, D, out_t=ref, stream=stream)
        torch.cuda.synchronize(dev)
    dist.broadcast(ref, 0)
    got = sharding.match_rowband(m, Lc, Rc, r, D, rank, world, out_t=d1, stream=stream)
    torch.cuda.synchronize(dev)
    bad = torch.tensor([float((got != ref).sum().item())], dtype=torch.float64, device=dev)
    dist.all_reduce(bad, op=dist.ReduceOp.MAX)
    band_check = {"parity": int(bad.item()) == 0, "rule": "bit-exact vs rank 0's single-GPU map, every rank",
                  "mismatching_pixels_max_over_ranks": int(bad.item())}

    def bstep():
        sharding.match_rowband(m, Lc, Rc, r, D, rank, world, out_t=d1, stream=stream)

    for _ in range(5):
        bstep()
    torch.cuda.synchronize(dev)
    dist.barrier()
    t1 = time.perf_counter()
    for _ in range(n):
        bstep()
    torch.cuda.synchronize(dev)
    dist.barrier()
    dt = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    rowband = {"value": round(n / float(dt.item()), 2), "unit": "disparity-maps/s",
               "ms_per_frame": round(float(dt.item()) * 1000 / n, 4), "collective": f"all_gather uint8 bands ({backend})",
               "halo_rows": r, "scaling": "strong", "check": band_check}

    return dslice, rowband


def main():
    args = parse()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be at least 1 and --warmup at least 0")
    if args.profile:
        args.full = args.no_cpu_baseline = args.no_variants = args.no_latency = args.no_cfg5 = True
    full = args.full
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # CPU baselines first, before this process initialises the GPU (the all-cores leg forks)
    cpu = cpu_all = None
    if full and not args.no_cpu_baseline and world == 1:
        cpu = cpu_baseline(args.width, args.height, args.num_disp, args.radius, args.seed)
        cpu_all = cpu_baseline_all_cores(args.width, args.height, args.num_disp, args.radius, args.seed)
    distributed = world > 1
    # one GPU per rank; SM_DIST_BACKEND=gloo with more ranks than GPUs is a rehearsal mode (ranks
    # share devices, collectives go through the host) for boxes with fewer GPUs than ranks
    backend = os.environ.get("SM_DIST_BACKEND", "nccl")
    dev_index = local_rank % max(1, torch.cuda.device_count()) if backend != "nccl" else local_rank
    dev = torch.device("cuda", dev_index)
    torch.cuda.set_device(dev)
    if distributed:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    import gpu_stereo_matching_amd as sm

    W, H, D, r, B = args.width, args.height, args.num_disp, args.radius, args.batch
    m = sm.BlockMatcher(dev_index, W, H, 256)

    # synthetic frames for this rank: seeds seed + global frame index (disjoint per rank)
    Ls, Rs = synth_batch(sm, args.seed + rank * B, B, W, H, D)
    Lt = torch.from_numpy(Ls).to(dev)
    Rt = torch.from_numpy(Rs).to(dev)
    del Ls, Rs
    out = torch.empty_like(Lt)
    stream = torch.cuda.current_stream(dev)

    def step():
        m.match_device(Lt, Rt, r, D, out_t=out, stream=stream)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(dev)

    # --full: per-launch kernel timing on the launch stream (one launch per step)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.steps if full else 0)]
    if distributed:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if full:
        for k in range(args.steps):
            ev[k][0].record(stream)
            step()
            ev[k][1].record(stream)
    else:
        for k in range(args.steps):
            step()
    torch.cuda.synchronize(dev)
    if distributed:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev])) if ev else None

    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    frames_total = B * world * args.steps
    value = frames_total / elapsed
    ms_per_step = elapsed * 1000.0 / args.steps

    if args.dump_outputs:
        dump_outputs(torch, args.dump_outputs, out, rank, world)

    # ---- single-frame latency (batch 1, device resident) ----
    lat = None
    if full and rank == 0 and not args.no_latency:
        o1 = torch.empty_like(Lt[0])
        for _ in range(5):
            m.match_device(Lt[0], Rt[0], r, D, out_t=o1, stream=stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(50):
            m.match_device(Lt[0], Rt[0], r, D, out_t=o1, stream=stream)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        lat = e0.elapsed_time(e1) / 50

    # ---- d-slice sharding of one frame (N > 1): cfg4, 1080p d_max=256, MIN reduction of the slice keys ----
    dslice = rowband = inventory = None
    if full and distributed:
        try:
            inventory = rank_inventory(torch, dist, dev, backend)
        except Exception as e:  # report, never hide
            inventory = {"error": f"{type(e).__name__}: {e}"}
        try:
            # one common frame (the same seed on every rank), not this rank's Lt[0]
            Lc_np, Rc_np = sm.synth_pair(args.seed, W, H, 256)
            Lc, Rc = torch.from_numpy(Lc_np).to(dev), torch.from_numpy(Rc_np).to(dev)
            dslice, rowband = run_split_extras(sm, torch, dist, m, Lc, Rc, W, H, D, r, rank, world, dev, stream,
                                               backend, args.steps)
        except Exception as e:  # report, never hide; the headline above is already measured
            dslice = {"error": f"{type(e).__name__}: {e}"}

    # ---- cfg5 as BASELINE configs[4] writes it: 4K pairs, d_max=192, guided + LR, frames batched
    #      over every rank (frame-parallel, no collective), whole-job maps/s with the max-over-ranks clock ----
    cfg5 = None
    if full and not args.no_cfg5:
        W5, H5, D5, B5 = 3840, 2160, 192, 8
        m5 = sm.BlockMatcher(dev_index, W5, H5, 256)
        try:
            p5 = [sm.synth_pair(4321 + rank * B5 + i, W5, H5, D5) for i in range(B5)]
            L5 = torch.from_numpy(np.stack([p[0] for p in p5])).to(dev)
            R5 = torch.from_numpy(np.stack([p[1] for p in p5])).to(dev)
            o5 = torch.empty_like(L5)

            def step5():
                m5.match_device(L5, R5, r, D5, out_t=o5, agg="guided", lr_check=True, stream=stream)

            for _ in range(2):
                step5()
            n5 = max(5, args.steps // 10)
            if distributed:
                dist.barrier()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for _ in range(n5):
                step5()
            torch.cuda.synchronize(dev)
            if distributed:
                dist.barrier()
            dt5 = time.perf_counter() - t1
            if distributed:
                t = torch.tensor([dt5], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt5 = float(t.item())
            cfg5 = {"config": f"cfg5: {W5}x{H5} synthetic pairs (seeds 4321+frame), {2*r+1}x{2*r+1} guided-filter "
                              f"aggregation + LR check, d_max={D5}, {B5} frames per launch per GPU, frame-parallel "
                              f"x{world}", "value": round(B5 * world * n5 / dt5, 2), "unit": "disparity-maps/s",
                    "ms_per_step": round(dt5 * 1000 / n5, 4), "steps": n5, "n_gpus": world, "scaling": "weak",
                    "kernel": "guided_fused_kernel<5, true>", "dtype": "fp32 (u8 in/out)"}
            if distributed:
                try:
                    # the north star's split on the configuration it pays for: ONE 4K guided + LR
                    # frame d-sharded over the ranks, left and right keys through two MIN reduce-scatters, the
                    # LR check on the gathered maps (sharding.match_dslice(lr_check=True))
                    from gpu_stereo_matching_amd import sharding
                    m5.set_guided_eps(1e-4 * 255 * 255)
                    kb5 = sharding.dslice_buffers(H5, W5, world, dev)
                    rb5 = sharding.dslice_buffers(H5, W5, world, dev)
                    # the same frame on every rank (seed 4321, frame 0 of rank 0's batch)
                    Lc5_np, Rc5_np = sm.synth_pair(4321, W5, H5, D5)
                    Lc5, Rc5 = torch.from_numpy(Lc5_np).to(dev), torch.from_numpy(Rc5_np).to(dev)
                    chk5 = split_parity_guided_lr(sm, torch, dist, m5, Lc5, Rc5, r, D5, rank, world, dev, stream)

                    def dstep5():
                        sharding.match_dslice(m5, Lc5, Rc5, r, D5, rank, world, keys_t=kb5[0], out_t=kb5[1],
                                              stream=stream, agg="guided", lr_check=True, right_bufs=rb5)

                    for _ in range(2):
                        dstep5()
                    torch.cuda.synchronize(dev)
                    dist.barrier()
                    t1 = time.perf_counter()
                    for _ in range(n5):
                        dstep5()
                    torch.cuda.synchronize(dev)
                    dist.barrier()
                    t = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    cfg5["dslice_guided_lr"] = {
                        "config": f"cfg5 one {W5}x{H5} frame, guided + LR, d_max={D5}, d-sharded over {world} ranks: "
                                  f"left + right slice keys, two MIN reduce_scatter int32 + two all_gather uint8 "
                                  f"({backend}), LR check", "value": round(n5 / float(t.item()), 2),
                        "unit": "disparity-maps/s", "ms_per_frame": round(float(t.item()) * 1000 / n5, 4),
                        "scaling": "strong", "keys_bytes_per_frame": W5 * H5 * 8, "check": chk5}
                except Exception as e:  # report, never hide
                    cfg5["dslice_guided_lr"] = {"error": f"{type(e).__name__}: {e}"}
        finally:
            m5.close()

    # ---- BASELINE configs, LR and guided variants on rank 0 ----
    variants = None
    if full and rank == 0 and not args.no_variants:
        variants = run_variants(sm, torch, dev, stream, args.seed)

    if rank == 0:
        bpm = algorithmic_bytes_per_map(W, H, D)
        roof = counts = None
        if full:
            eq_hbm = bpm * B / (kern_ms * 1e-3) / 1e9
            traffic = None
            try:
                with open(args.pmc_json) as f:
                    pm = json.load(f)
                if pm.get("workload") == [W, H, D, r, B]:
                    traffic = pm.get("hbm_bytes_per_launch")
            except (OSError, ValueError):
                pass
            counts = load_counts(args.valu_json)
            roof = valu_roofline(counts, f"box_r5_1080p_d128_b{B}", [W, H, D, r, B], kern_ms, f"box_match_kernel<{r}>", {
                "traffic": traffic,
                "traffic_frac_of_hbm_peak": round(traffic / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if traffic else None,
                "equivalent_hbm_frac": round(eq_hbm / HBM_PEAK_GBS, 4),
                "algorithmic_bytes_per_launch": bpm * B,
                "note": "bound = VALU issue (the fused kernel reads the pair and writes the map: measured HBM traffic is "
                        "the compulsory 3P bytes, traffic_frac_of_hbm_peak); equivalent_hbm_frac = P*(2D+3) bytes per "
                        "map (SURVEY §8d, the reference's AD-volume data flow, never materialised here) / launch time / "
                        "8 TB/s: a speed figure, not a roofline fraction (DESIGN.md §8)"})
        res = {
            "metric": "disparity-maps/sec + ms/frame, 1080p d_max=128",
            "value": round(value, 2),
            "unit": "disparity-maps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "ms_per_frame": round(ms_per_step / B, 4),             # per-GPU throughput time (value's inverse at N=1)
            "latency_ms_batch1": round(lat, 4) if lat is not None else None,   # one frame per launch
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "config": {
                "workload": f"cfg3: {W}x{H} synthetic rectified pairs, {2*r+1}x{2*r+1} SAD box aggregation + WTA "
                            f"(bit-exact with getDisp/kernalFindCorr), d_max={D}; the path BASELINE.md's GPU-target "
                            f"table and the north star's >=100x CPU BlockMatching.cpp target are quoted on; "
                            f"BASELINE configs[2]'s guided-filter aggregation of the same frames: 'cfg3_guided'",
                "width": W, "height": H, "num_disp": D, "radius": r, "frames_per_step_per_gpu": B,
                "seed": args.seed, "parallelism": f"frame-parallel x{world}",
            },
            "roofline": roof,
            "cpu_baseline": cpu,
            "cpu_baseline_all_cores": cpu_all,
        }
        if inventory is not None:
            res["rccl_world"] = inventory
            checks = [c.get("check", {}).get("parity") for c in (dslice or {}, rowband or {})]
            checks.append(((cfg5 or {}).get("dslice_guided_lr") or {}).get("check", {}).get("parity"))
            res["split_parity"] = all(c is True for c in checks) if None not in checks else None
        if dslice is not None:
            res["dslice"] = dslice
        if rowband is not None:
            res["rowband"] = rowband
        if cfg5 is not None:
            res["cfg5_guided_lr"] = cfg5
        if variants:
            res["variants"] = variants
            # BASELINE configs[2] as written (11x11 + guided-filter aggregation, 1080p d_max=128),
            # the same synthetic frames, 4 per launch; no CPU port of the guided path is timed here
            # (the fp64 oracle takes ~17 s per 1080p map on one core: tests/test_gpu_guided.py)
            g = variants.get("cfg3 1080p 11x11 guided d128", {})
            glr = variants.get("cfg3 1080p 11x11 guided+lr d128", {})
            if "maps_per_s" in g:
                res["cfg3_guided"] = {"value": g["maps_per_s"], "unit": "disparity-maps/s",
                                      "ms_per_frame": g["ms_per_frame"], "frames_per_step": g["frames_per_call"],
                                      "with_lr_check": {"value": glr.get("maps_per_s"),
                                                        "ms_per_frame": glr.get("ms_per_frame")},
                                      "kernel": "guided_fused_kernel<5>", "dtype": "fp32 (u8 in/out)"}
                res["cfg3_guided"]["roofline"] = valu_roofline(
                    counts, "guided_r5_1080p_d128_b32", [1920, 1080, 128, 5, g["frames_per_call"]],
                    g["ms_per_frame"] * g["frames_per_call"], "guided_fused_kernel<5, false>",
                    {"equivalent_hbm_frac": round(bpm / (g["ms_per_frame"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
                if "maps_per_s" in glr:
                    res["cfg3_guided"]["with_lr_check"]["roofline"] = valu_roofline(
                        counts, "guided_lr_r5_1080p_d128_b32", [1920, 1080, 128, 5, glr["frames_per_call"]],
                        glr["ms_per_frame"] * glr["frames_per_call"], "guided_fused_kernel<5, true> (+ right-key "
                        "reduction and LR check in the launch time)")
            st = variants.get("staged kernels 1080p d128 (HBM roofline per kernel)")
            if st:
                res["staged_hbm_roofline"] = st
        print(json.dumps(res), flush=True)

    m.close()
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
