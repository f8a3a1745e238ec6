"""GPU: on-device 2-NN descriptor matching with the reference's ratio test (feature_matcher::match_two_image,
feature_matcher.cpp:42-59) and the uploads straight from its matches.

Exactness is judged against an f64 numpy brute force with the tie window of DESIGN.md section 3.10:
w = 2 D 2^-24 (|q|^2 + |t|^2) bounds the f32 error of both the ranking score and the rescored squared distance, so two
candidates whose f64 squared distances differ by less than w may legitimately swap, and a reported distance may differ
from the f64 one by that much (in squared terms)."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu


def _window(q, t):
    D = q.shape[1]
    return 2 * D * 2.0**-24 * ((q.astype(np.float64) ** 2).sum(1)[:, None] + (t.astype(np.float64) ** 2).sum(1)[None, :])


def _brute(q, t):
    """f64 squared distances (nq, nt)."""
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    return (q64 ** 2).sum(1)[:, None] + (t64 ** 2).sum(1)[None, :] - 2.0 * q64 @ t64.T


def _check_against_numpy(q, t, m, ratio=0.3):
    nq, nt = q.shape[0], t.shape[0]
    d2 = np.maximum(_brute(q, t), 0.0)
    w = _window(q, t)
    rows = np.arange(nq)
    order = np.argsort(d2, axis=1, kind="stable")
    i0, i1 = order[:, 0], order[:, 1]
    g0, g1 = m.nn_index[:, 0], m.nn_index[:, 1]
    assert (g0 >= 0).all() and (g1 >= 0).all() and (g0 != g1).all()
    # the chosen neighbours are the true ones up to the window
    for gi, ti in ((g0, i0), (g1, i1)):
        bad = gi != ti
        assert (np.abs(d2[rows, gi] - d2[rows, ti]) <= w[rows, gi] + w[rows, ti])[bad].all(), np.flatnonzero(bad)[:5]
    # reported distances (squared) within the window of the f64 ones
    for k, gi in enumerate((g0, g1)):
        err = np.abs(m.nn_distance[:, k].astype(np.float64) ** 2 - d2[rows, gi])
        assert (err <= 2 * w[rows, gi] + 1e-30).all(), err.max()
    # ratio decisions: agree except within the window of the boundary
    d0, d1 = np.sqrt(d2[rows, i0]), np.sqrt(d2[rows, i1])
    want = d0 < ratio * d1
    got = np.zeros(nq, bool)
    got[m.query_idx] = True
    margin = np.abs(d2[rows, i0] - ratio**2 * d2[rows, i1])
    near = margin <= 4 * (w[rows, i0] + w[rows, i1])
    assert (got == want)[~near].all()
    assert np.array_equal(m.query_idx, np.sort(m.query_idx))
    assert np.array_equal(m.train_idx, m.nn_index[m.query_idx, 0])
    assert np.array_equal(m.distance, m.nn_distance[m.query_idx, 0])
    return want


def _descriptors(rng, n, D, padded):
    if not padded:
        return rng.standard_normal((n, D)).astype(np.float32)
    wide = rng.standard_normal((n, D + 7)).astype(np.float32)
    return wide[:, :D]                      # a row stride of 4 (D + 7) bytes, like a cv::Mat with a larger step


@pytest.mark.parametrize("D", [64, 128, 36])
@pytest.mark.parametrize("nq,nt", [(1, 2), (31, 33), (127, 129), (1000, 3000), (4097, 2049)])
def test_against_numpy_brute_force(D, nq, nt):
    rng = np.random.default_rng(nq * 7919 + nt * 31 + D)
    padded = (nq + D) % 2 == 1
    q = _descriptors(rng, nq, D, padded)
    t = _descriptors(rng, nt, D, padded)
    # a few near-duplicates so that the ratio test accepts something
    k = min(nq, nt) // 3
    q[:k] = t[:k] + 0.05 * rng.standard_normal((k, D)).astype(np.float32)
    m = api.match_descriptors(q, t)
    _check_against_numpy(q, t, m)


def test_unit_descriptors_dim_256_and_200():
    rng = np.random.default_rng(3)
    for D in (256, 200):
        t = rng.standard_normal((700, D)).astype(np.float32)
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        q = t[rng.permutation(700)[:300]] + 0.01 * rng.standard_normal((300, D)).astype(np.float32)
        _check_against_numpy(q, t, api.match_descriptors(q, t))


def test_planted_matches_are_found():
    pm = synthetic.planted_matches(3000, distractors_left=1500, distractors_right=2500, seed=11)
    m = api.match_descriptors(pm.left_desc, pm.right_desc)
    want = _check_against_numpy(pm.left_desc, pm.right_desc, m)
    got = dict(zip(m.query_idx.tolist(), m.train_idx.tolist()))
    for l, r in zip(pm.planted_left.tolist(), pm.planted_right.tolist()):
        assert got.get(l) == r
    assert np.array_equal(np.flatnonzero(want), m.query_idx)       # the accepted set is numpy's
    assert np.all(np.diff(m.query_idx) > 0)


def test_ties_and_degenerate_input():
    rng = np.random.default_rng(5)
    t = rng.standard_normal((100, 64)).astype(np.float32)
    t[70] = t[20]                                      # duplicate train rows: the lower index wins, the ratio test fails
    q = t[[20, 5]] + 0.0
    m = api.match_descriptors(q, t)
    assert m.nn_index[0].tolist() == [20, 70] and m.nn_distance[0, 0] == 0.0 and m.nn_distance[0, 1] == 0.0
    assert m.query_idx.tolist() == [1] and m.train_idx.tolist() == [5]
    for nt in (0, 1):
        m = api.match_descriptors(q, t[:nt])
        assert m.query_idx.size == 0 and (m.nn_index[:, 1] == -1).all()
        assert (m.nn_index[:, 0] == (0 if nt else -1)).all()
    m = api.match_descriptors(np.zeros((0, 64), np.float32), t)
    assert m.query_idx.size == 0 and m.nn_index.shape == (0, 2)
    # NaN rows: a query with one matches nothing, a train row with one is never chosen
    t2 = t.copy()
    t2[5, 3] = np.nan
    q2 = t[[5, 6, 7]].copy()
    q2[1, 0] = np.inf
    m = api.match_descriptors(q2, t2)
    assert (m.nn_index[:, :] != 5).all()
    assert m.nn_index[1].tolist() == [-1, -1] and np.isinf(m.nn_distance[1]).all()
    assert 1 not in m.query_idx.tolist() and m.nn_index[2, 0] == 7 and 2 in m.query_idx.tolist()


def test_exact_ties_across_lane_halves_and_splits():
    """Equal scores met by the lexicographic merges: rows 0 and 4 of a tile sit in different lane halves (half-wave merge);
    rows 0 and n - 1 of 20 k train rows against one query sit in different train splits (per-split merge)."""
    rng = np.random.default_rng(9)
    t = rng.standard_normal((100, 64)).astype(np.float32)
    t[4] = t[0]
    m = api.match_descriptors(t[[0, 4]], t)
    assert m.nn_index.tolist() == [[0, 4], [0, 4]] and m.query_idx.size == 0
    t[4] = t[0] + 0.5                    # the copy at the higher index ranks second, not first
    t[36] = t[0]
    m = api.match_descriptors(t[[36]], t)
    assert m.nn_index.tolist() == [[0, 36]]
    n = 20000
    t = rng.standard_normal((n, 64)).astype(np.float32)
    t[n - 1] = t[0]
    t[n // 2] = t[0]
    for k in (1, 3):                     # one query: 64 splits of the train tiles
        m = api.match_descriptors(np.repeat(t[[n - 1]], k, axis=0), t)
        assert (m.nn_index == [0, n // 2]).all() and m.query_idx.size == 0
    t[n // 2] += 1.0
    m = api.match_descriptors(t[[n - 1]], t)
    assert m.nn_index.tolist() == [[0, n - 1]]


def test_deterministic_and_independent_of_the_other_queries_and_the_split():
    rng = np.random.default_rng(17)
    t = rng.standard_normal((20000, 64)).astype(np.float32)
    q = np.concatenate([t[:3000] + 0.1 * rng.standard_normal((3000, 64)).astype(np.float32),
                        rng.standard_normal((3000, 64)).astype(np.float32)])
    a, b = api.match_descriptors(q, t), api.match_descriptors(q, t)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for k in (1, 37, 300):           # few queries: the train rows are split over many blocks
        s = api.match_descriptors(q[:k], t)
        assert np.array_equal(s.nn_index, a.nn_index[:k]) and np.array_equal(s.nn_distance, a.nn_distance[:k])
        assert np.array_equal(s.query_idx, a.query_idx[a.query_idx < k])
    # a ragged batch, empty pairs included, equals the single-pair calls
    nqs, nts = [500, 0, 3000, 1, 257, 40, 0], [2000, 100, 7000, 5, 0, 1, 0]
    qo, to = np.concatenate([[0], np.cumsum(nqs)]), np.concatenate([[0], np.cumsum(nts)])
    Q = rng.standard_normal((qo[-1], 64)).astype(np.float32)
    T = rng.standard_normal((to[-1], 64)).astype(np.float32)
    Q[:300] = T[:300] + 0.05 * rng.standard_normal((300, 64)).astype(np.float32)
    bm = api.batch_match_descriptors(Q, qo, T, to)
    for g in range(len(nqs)):
        s = api.match_descriptors(Q[qo[g]:qo[g + 1]], T[to[g]:to[g + 1]])
        assert np.array_equal(bm.nn_index[qo[g]:qo[g + 1]], s.nn_index)
        assert np.array_equal(bm.nn_distance[qo[g]:qo[g + 1]], s.nn_distance)
        lo, hi = bm.match_offsets[g], bm.match_offsets[g + 1]
        assert bm.n_matched[g] == s.query_idx.size
        assert np.array_equal(bm.query_idx[lo:hi], s.query_idx) and np.array_equal(bm.train_idx[lo:hi], s.train_idx)
        assert np.array_equal(bm.distance[lo:hi], s.distance)


def test_full_size_50k_sample():
    rng = np.random.default_rng(23)
    n, D = 50000, 64
    t = rng.standard_normal((n, D)).astype(np.float32)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    q = rng.standard_normal((n, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[: n // 2] = t[rng.permutation(n)[: n // 2]] + 0.02 * rng.standard_normal((n // 2, D)).astype(np.float32)
    m = api.match_descriptors(q, t)
    sample = np.sort(rng.choice(n, 2000, replace=False))
    sub = api.Matches(m.nn_index[sample], m.nn_distance[sample], *(np.zeros(0, np.int32),) * 2, np.zeros(0, np.float32))
    d2 = np.maximum(_brute(q[sample], t), 0.0)
    w = _window(q[sample], t)
    rows = np.arange(sample.size)
    order = np.argsort(d2, axis=1, kind="stable")
    for k in range(2):
        gi, ti = sub.nn_index[:, k], order[:, k]
        assert (np.abs(d2[rows, gi] - d2[rows, ti]) <= w[rows, gi] + w[rows, ti]).all()
        assert (np.abs(sub.nn_distance[:, k].astype(np.float64) ** 2 - d2[rows, gi]) <= 2 * w[rows, gi]).all()
    accepted = np.zeros(n, bool)
    accepted[m.query_idx] = True
    d0, d1 = d2[rows, order[:, 0]], d2[rows, order[:, 1]]
    near = np.abs(d0 - 0.09 * d1) <= 4 * (w[rows, order[:, 0]] + w[rows, order[:, 1]])
    assert (accepted[sample] == (np.sqrt(d0) < 0.3 * np.sqrt(d1)))[~near].all()


def _host_gathered(pm, m):
    return pm.left_kp[m.query_idx], pm.right_kp[m.train_idx]


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32])
def test_problem_upload_matches_postcondition(store):
    pm = synthetic.planted_matches(2500, 800, 1200, seed=31, sigma=2e-4, outlier_fraction=0.02)
    m = api.match_descriptors(pm.left_desc, pm.right_desc)
    kl, kr = _host_gathered(pm, m)
    rot, tran = pm.geometry.rot_init, pm.geometry.tran_init
    for depth in (None, 6.0):
        d12 = None if depth is None else np.full((kl.shape[0], 2), depth)
        with api.Problem(0) as a, api.Problem(0) as b:
            ml, mr = a.upload_matches(pm.left_kp, pm.right_kp, pm.left_desc, pm.right_desc, pm.im_width, pm.im_height,
                                      init_depth=depth, store=store)
            b.upload_keypoints(kl, kr, pm.im_width, pm.im_height, d12=d12, store=store)
            assert np.array_equal(ml, m.query_idx) and np.array_equal(mr, m.train_idx)
            assert a.size == b.size == m.query_idx.size
            dms = [api.DEPTH_UNIFORM] + ([api.DEPTH_PER_MATCH] if depth is not None else [])
            for mode in (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT):
                for dm in dms:
                    pa = a.eval_pack(mode, rot, tran, 5.0, 7.0, depth_mode=dm)
                    pb = b.eval_pack(mode, rot, tran, 5.0, 7.0, depth_mode=dm)
                    assert np.array_equal(pa, pb), (mode, dm)


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32])
def test_batch_upload_matches_postcondition(store):
    pms = [synthetic.planted_matches(n, dl, dr, seed=40 + i) for i, (n, dl, dr) in
           enumerate([(1500, 200, 900), (0, 30, 50), (800, 0, 0), (0, 0, 0), (2100, 700, 300)])]
    lo = np.concatenate([[0], np.cumsum([p.left_kp.shape[0] for p in pms])])
    ro = np.concatenate([[0], np.cumsum([p.right_kp.shape[0] for p in pms])])
    KL = np.concatenate([p.left_kp for p in pms]); KR = np.concatenate([p.right_kp for p in pms])
    DL = np.concatenate([p.left_desc for p in pms]); DR = np.concatenate([p.right_desc for p in pms])
    W, H = pms[0].im_width, pms[0].im_height
    depths = np.array([4.0, 5.0, 6.0, 7.0, 8.0])
    x1, x2, d12, counts = [], [], [], []
    for g, p in enumerate(pms):
        s = api.match_descriptors(p.left_desc, p.right_desc)
        x1.append(api.keypoints_to_sphere(p.left_kp[s.query_idx], W, H).reshape(-1, 3))
        x2.append(api.keypoints_to_sphere(p.right_kp[s.train_idx], W, H).reshape(-1, 3))
        d12.append(np.full((s.query_idx.size, 2), depths[g]))
        counts.append(s.query_idx.size)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    B = len(pms)
    rot = np.stack([p.geometry.rot_init for p in pms]); tran = np.stack([p.geometry.tran_init for p in pms])
    for depth in (None, depths):
        with api.Batch(0) as a, api.Batch(0) as b:
            ml, mr, n = a.upload_matches(KL, lo, KR, ro, DL, DR, W, H, init_depth=depth, store=store)
            b.upload(np.concatenate(x1), np.concatenate(x2), off, None if depth is None else np.concatenate(d12), store=store)
            assert np.array_equal(n, counts) and np.array_equal(a.offsets, b.offsets)
            dms = [api.DEPTH_UNIFORM] + ([api.DEPTH_PER_MATCH] if depth is not None else [])
            for mode in (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT):
                for dm in dms:
                    pa = a.eval(mode, rot, tran, np.full(B, 5.0), np.full(B, 7.0), depth_mode=dm)
                    pb = b.eval(mode, rot, tran, np.full(B, 5.0), np.full(B, 7.0), depth_mode=dm)
                    assert np.array_equal(pa, pb), (mode, dm)


def test_batch_end_to_end_on_planted_pairs():
    pms = [synthetic.planted_matches(n, n // 3, n // 2, seed=60 + i, sigma=2e-4, outlier_fraction=0.02)
           for i, n in enumerate([3000, 2048, 1500, 4097])]
    lo = np.concatenate([[0], np.cumsum([p.left_kp.shape[0] for p in pms])])
    ro = np.concatenate([[0], np.cumsum([p.right_kp.shape[0] for p in pms])])
    KL = np.concatenate([p.left_kp for p in pms]); KR = np.concatenate([p.right_kp for p in pms])
    DL = np.concatenate([p.left_desc for p in pms]); DR = np.concatenate([p.right_desc for p in pms])
    W, H = pms[0].im_width, pms[0].im_height
    with api.Batch(0) as a:
        ml, mr, n = a.upload_matches(KL, lo, KR, ro, DL, DR, W, H, init_depth=6.0)
        off = a.offsets.astype(np.int64)
        res = a.solve_problem(seed=5)
    x1 = np.concatenate([api.keypoints_to_sphere(p.left_kp[ml[off[g]:off[g + 1]]], W, H).reshape(-1, 3) for g, p in enumerate(pms)])
    x2 = np.concatenate([api.keypoints_to_sphere(p.right_kp[mr[off[g]:off[g + 1]]], W, H).reshape(-1, 3) for g, p in enumerate(pms)])
    with api.Batch(0) as b:
        b.upload(x1, x2, off.astype(np.uint64), np.full((x1.shape[0], 2), 6.0))
        res2 = b.solve_problem(seed=5)
    assert (res["status"] == 0).all()
    assert np.array_equal(res["rot"], res2["rot"]) and np.array_equal(res["tran"], res2["tran"])
    for g, p in enumerate(pms):
        assert n[g] >= p.planted_left.size * 0.99
        assert np.abs(res["rot"][g] - p.geometry.rot_true).max() < 0.15, g


SBA_MAIN = ROOT / "spherical_bundle_adjuster_amd" / "csrc" / "build" / "sba_main"


def _write_kp(path, kp, W, H, desc=None):
    with open(path, "wb") as f:
        np.array([kp.shape[0], W, H, 0 if desc is None else desc.shape[1]], dtype=np.int32).tofile(f)
        np.ascontiguousarray(kp, np.float32).tofile(f)
        if desc is not None:
            np.ascontiguousarray(desc, np.float32).tofile(f)


def _run_cli(tmp, left, right, c):
    args = [str(SBA_MAIN), str(left), str(right), *(f"{v:.17g}" for v in np.rad2deg(c.rot_init)),
            *(f"{v:.17g}" for v in c.tran_init), "6"]
    r = subprocess.run(args, cwd=tmp, capture_output=True, text=True, timeout=120, env=dict(os.environ, SBA_INITIAL_GUESS="0"))
    assert r.returncode == 0, r.stderr + r.stdout
    return (tmp / "log.txt").read_text().strip().splitlines()[-1], r.stdout


def test_cli_descriptor_files_match_first(tmp_path):
    """sba_main on key-point files with D = 64 descriptors (different counts on the two sides) -- the mirror class's
    do_bundle_adjustment_from_features -- writes the log.txt row of sba_main on the matched records match_descriptors
    selects."""
    assert SBA_MAIN.exists(), "build with make -C spherical_bundle_adjuster_amd/csrc"
    pm = synthetic.planted_matches(2048, 500, 900, seed=77, sigma=2e-4, outlier_fraction=0.02)
    W, H = pm.im_width, pm.im_height
    a, b = tmp_path / "desc", tmp_path / "matched"
    a.mkdir(); b.mkdir()
    _write_kp(a / "left.kp", pm.left_kp, W, H, pm.left_desc)
    _write_kp(a / "right.kp", pm.right_kp, W, H, pm.right_desc)
    row_desc, out = _run_cli(a, a / "left.kp", a / "right.kp", pm.geometry)
    m = api.match_descriptors(pm.left_desc, pm.right_desc)
    assert m.query_idx.size >= 2048 and f"matched : {m.query_idx.size}" in out
    _write_kp(b / "left.kp", pm.left_kp[m.query_idx], W, H)
    _write_kp(b / "right.kp", pm.right_kp[m.train_idx], W, H)
    row_matched, _ = _run_cli(b, b / "left.kp", b / "right.kp", pm.geometry)
    assert row_desc == row_matched
    assert int(row_desc.split(",")[9]) == m.query_idx.size
    got_rot = np.deg2rad([float(v) for v in row_desc.split(",")[3:6]])
    assert np.abs(got_rot - pm.geometry.rot_true).max() < 0.15
