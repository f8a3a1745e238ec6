"""Workload of tools/profile_landmark_associate.sh: the association of a frame with a described landmark map at a map-sized
shape, next to the matcher alone on the same device arrays and the host route the association replaces (match, numpy unique,
sort, upload); then a prune of half a described map next to the same prune undescribed.  Prints one JSON line with the wall
times in ms (each the best of CALLS after one warm-up call); the kernels are timed by the trace around this script.

usage: landmark_associate_workload.py [N_MAP [M_FRAME [DIM [N_PRUNE [CALLS]]]]]"""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import _cabi as cabi  # noqa: E402
from spherical_bundle_adjuster_amd import api  # noqa: E402


def best_ms(fn, calls):
    fn()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return min(times)


def rows(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.normal(size=(n, 3)) + np.array([0.0, 0.0, 6.0])
    cov = np.zeros((n, 6))
    cov[:, :3] = 1e-3
    return xyz, cov


def main():
    n, m, dim, n_prune, calls = (int(a) for a in (sys.argv[1:] + ["1000000", "8192", "64", "10000000", "5"][len(sys.argv) - 1:]))
    dev = torch.device("cuda:0")
    lib = cabi.load_library()
    rng = np.random.default_rng(1)
    desc = rng.integers(-8, 9, size=(n, dim)).astype(np.float32)
    seen = rng.permutation(n)[:m // 2]                                   # half of the frame: landmarks moved by +-1 in one entry
    frame = rng.integers(-8, 9, size=(m, dim)).astype(np.float32)
    frame[:len(seen)] = desc[seen]
    frame[np.arange(len(seen)), rng.integers(0, dim, len(seen))] += 1.0
    y = rng.normal(size=(m, 3))
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    out = {"n": n, "m": m, "dim": dim, "n_prune": n_prune, "calls": calls}
    with api.Landmarks(0) as L:
        L.set(*rows(n, 2))
        L.set_descriptors(desc)
        f_dev, d_dev, y_dev = torch.from_numpy(frame).to(dev), torch.from_numpy(desc).to(dev), torch.from_numpy(y).to(dev)
        b_out = torch.zeros(3 * m, dtype=torch.float64, device=dev)
        nn_i = torch.zeros(2 * m, dtype=torch.int32, device=dev)
        nn_d = torch.zeros(2 * m, dtype=torch.float32, device=dev)
        mq, mt, md = (torch.zeros(m, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.float32))
        torch.cuda.synchronize()
        a = L.associate_device(f_dev.data_ptr(), m, dim, y_dev.data_ptr(), b_out.data_ptr())
        out.update(n_accepted=a.n_accepted, n_associated=a.n_associated, n_contested=a.n_contested)
        out["associate_device_ms"] = best_ms(lambda: L.associate_device(f_dev.data_ptr(), m, dim, y_dev.data_ptr(), b_out.data_ptr()), calls)
        out["associate_host_ms"] = best_ms(lambda: L.associate(frame, y), calls)
        n_matched = C.c_size_t(0)

        def match_alone():
            cabi.check(lib, lib.sba_match_descriptors_device(0, None, C.c_void_p(f_dev.data_ptr()), m, C.c_void_p(d_dev.data_ptr()), n, dim, 4 * dim,
                                                             0.3, C.c_void_p(nn_i.data_ptr()), C.c_void_p(nn_d.data_ptr()), C.byref(n_matched),
                                                             C.c_void_p(mq.data_ptr()), C.c_void_p(mt.data_ptr()), C.c_void_p(md.data_ptr())))
        out["match_device_alone_ms"] = best_ms(match_alone, calls)

        def host_route():       # what a caller did before: match against the array kept beside the map, resolve, sort, upload
            r = api.match_descriptors(frame, desc, ratio=0.3)
            order = np.lexsort((r.query_idx, r.distance.view(np.uint32), r.train_idx))
            t = r.train_idx[order]
            first = np.ones(len(t), dtype=bool)
            first[1:] = t[1:] != t[:-1]
            win = order[first]
            idx = r.train_idx[win].astype(np.int64)
            b = torch.from_numpy(np.ascontiguousarray(y[r.query_idx[win]])).to(dev)
            torch.cuda.synchronize()
            return idx, b
        idx, _ = host_route()
        assert np.array_equal(idx, a.idx)
        out["host_route_ms"] = best_ms(host_route, calls)
    del desc, frame
    # a prune of half a map, described and not; the map is set again before every call (not timed)
    xyz, cov = rows(n_prune, 3)
    big = rng.integers(-8, 9, size=(n_prune, dim), dtype=np.int8).astype(np.float32)
    mask = rng.random(n_prune) < 0.5
    for name, described in (("prune_undescribed_ms", False), ("prune_described_ms", True)):
        with api.Landmarks(0) as L:
            times = []
            for _ in range(calls + 1):
                L.set(xyz, cov)
                if described:
                    L.set_descriptors(big)
                t0 = time.perf_counter()
                r = L.prune(mask=mask, want_kept=False)
                times.append(1e3 * (time.perf_counter() - t0))
            out[name] = min(times[1:])
            out["n_kept"] = r.n_kept
    print(json.dumps(out))


if __name__ == "__main__":
    main()
