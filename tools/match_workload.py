"""Descriptor-match workload: exact L2 2-NN + ratio test on the device (sba_match_descriptors_device) at the shapes of
DESIGN.md section 3.10, against a 16-thread CPU exact brute force for context.

Single pairs: the time of sba_match_descriptors_device (median of --reps, inputs already resident; it includes the packing,
the product, the finish and the compaction, and its one synchronisation), 2 Nq Nt D FLOP over that time, and the share of
the f32 matrix peak (157.3 TF).  The batch has only a host entry point: its figure is a HOST ROUND TRIP (about 1 GB of
pageable H2D copies included) and gets no TF figure; its kernel times, like the per-kernel split of every shape, come from
a rocprofv3 --kernel-trace --stats run of this tool (profiles/match_kernel_stats.csv).

Beside each shape: an exact 16-thread torch-CPU brute force (blocked f32 GEMM + top-2 + ratio test).  Above --cpu-max
queries it runs on a sample of --cpu-sample queries of the first pair and is extrapolated linearly in the query count.

    python tools/match_workload.py [--reps 5] [--cpu-max 20000] [--json out.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spherical_bundle_adjuster_amd import _cabi as cabi  # noqa: E402

PEAK_TF = 157.3
SHAPES = [  # (label, pairs, Nq, Nt, D)
    ("C1-like 2k x 2k", 1, 2048, 2048, 64),
    ("20k x 20k", 1, 20000, 20000, 64),
    ("50k x 50k D64", 1, 50000, 50000, 64),
    ("50k x 50k D128", 1, 50000, 50000, 128),
    ("batch 256 x 8k x 8k", 256, 8192, 8192, 64),
]


def _data(rng, pairs, nq, nt, D):
    import torch
    t = torch.randn(pairs * nt, D, generator=rng, device="cuda")
    t = t / t.norm(dim=1, keepdim=True)
    q = torch.randn(pairs * nq, D, generator=rng, device="cuda")
    q = q / q.norm(dim=1, keepdim=True)
    k = nq // 2          # half the queries are noisy copies of train rows of their own pair
    for g in range(pairs):
        q[g * nq: g * nq + k] = t[g * nt: g * nt + k] + 0.02 * torch.randn(k, D, generator=rng, device="cuda")
    return q.contiguous(), t.contiguous()


def _device_call(lib, q, t, nq, nt, D, outs):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    n = C.c_size_t()
    rc = lib.sba_match_descriptors_device(0, C.c_void_p(stream), C.c_void_p(q.data_ptr()), nq, C.c_void_p(t.data_ptr()), nt, D,
                                          4 * D, C.c_float(0.3), None, None, C.byref(n), C.c_void_p(outs[0].data_ptr()),
                                          C.c_void_p(outs[1].data_ptr()), C.c_void_p(outs[2].data_ptr()))
    cabi.check(lib, rc)
    return n.value


def _batch_call(lib, qh, th, pairs, nq, nt, D):
    qo = np.arange(pairs + 1, dtype=np.uint64) * nq
    to = np.arange(pairs + 1, dtype=np.uint64) * nt
    cnt = np.zeros(pairs, np.uint64)
    mq = np.zeros(pairs * nq, np.int32); mt = np.zeros(pairs * nq, np.int32); md = np.zeros(pairs * nq, np.float32)
    rc = lib.sba_batch_match_descriptors(0, C.c_void_p(qh.ctypes.data), C.c_void_p(qo.ctypes.data), C.c_void_p(th.ctypes.data),
                                         C.c_void_p(to.ctypes.data), pairs, D, 4 * D, C.c_float(0.3), None, None,
                                         C.c_void_p(cnt.ctypes.data), C.c_void_p(mq.ctypes.data), C.c_void_p(mt.ctypes.data),
                                         C.c_void_p(md.ctypes.data))
    cabi.check(lib, rc)
    return int(cnt.sum())


def _cpu_brute(q, t, threads=16):
    """Exact 2-NN by blocked f32 GEMM on torch-CPU (16 threads), ratio test 0.3."""
    import torch
    torch.set_num_threads(threads)
    qt, tt = torch.from_numpy(q), torch.from_numpy(t)
    tn = (tt * tt).sum(1)
    kept = 0
    for lo in range(0, qt.shape[0], 4096):
        s = tn[None, :] - 2.0 * qt[lo:lo + 4096] @ tt.T
        v, _ = torch.topk(s, 2, dim=1, largest=False)
        qn = (qt[lo:lo + 4096] ** 2).sum(1, keepdim=True)
        d = (v + qn).clamp_min(0).sqrt()
        kept += int((d[:, 0] < 0.3 * d[:, 1]).sum())
    return kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-max", type=int, default=20000, help="largest query count the CPU brute force runs in full")
    ap.add_argument("--cpu-sample", type=int, default=2048, help="queries of the sampled CPU brute force above --cpu-max (0: none)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="substring of the shape labels to run")
    a = ap.parse_args()
    import torch
    lib = cabi.load_library()
    rng = torch.Generator(device="cuda")
    rng.manual_seed(1234)
    rows = []
    for label, pairs, nq, nt, D in SHAPES:
        if a.only and a.only not in label:
            continue
        q, t = _data(rng, pairs, nq, nt, D)
        flop = 2.0 * pairs * nq * nt * D
        times = []
        if pairs == 1:
            outs = [torch.empty(nq, dtype=torch.int32, device="cuda"), torch.empty(nq, dtype=torch.int32, device="cuda"),
                    torch.empty(nq, dtype=torch.float32, device="cuda")]
            _device_call(lib, q, t, nq, nt, D, outs)           # warm-up
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = _device_call(lib, q, t, nq, nt, D, outs)
                times.append(time.perf_counter() - t0)
            what = "device call"
        else:
            qh, th = q.cpu().numpy(), t.cpu().numpy()
            _batch_call(lib, qh, th, pairs, nq, nt, D)
            for _ in range(a.reps):
                t0 = time.perf_counter()
                m = _batch_call(lib, qh, th, pairs, nq, nt, D)
                times.append(time.perf_counter() - t0)
            what = "host round trip"
        sec = float(np.median(times))
        device_timed = pairs == 1
        row = {"shape": label, "pairs": pairs, "nq": nq, "nt": nt, "dim": D, "matched": m, "seconds": sec, "timed": what,
               "tflops": flop / sec / 1e12 if device_timed else None,
               "peak_share": flop / sec / 1e12 / PEAK_TF if device_timed else None}
        cpu = ""
        if pairs * nq <= a.cpu_max or a.cpu_sample > 0:
            full = pairs * nq <= a.cpu_max
            k = nq if full else min(nq, a.cpu_sample)
            qc, tc = q[:k].cpu().numpy(), t[:nt].cpu().numpy()
            t0 = time.perf_counter()
            _cpu_brute(qc, tc)
            cs = (time.perf_counter() - t0) * (pairs * nq / k)
            row["cpu16_seconds"] = cs
            row["cpu16_extrapolated_from_queries"] = None if full else k
            cpu = f"  | cpu16 {cs * 1e3:10.1f} ms" + ("" if full else f" (from {k} queries)")
        rows.append(row)
        dev = (f"{row['tflops']:7.2f} TF  {100 * row['peak_share']:5.1f} % of f32 peak" if device_timed
               else "(incl. H2D of the inputs: no TF figure; kernel times in the trace)")
        print(f"{label:>22}: {sec * 1e3:9.3f} ms {what}  {dev}  matched {m}{cpu}", flush=True)
        del q, t
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
