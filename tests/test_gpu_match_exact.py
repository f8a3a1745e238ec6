"""GPU: the descriptor match on integer-valued descriptors, bit for bit.

Every f32 operation of the device path is exact on the cases of tests/match_cases.py (tests/test_match_cases_cpu.py shows
that they lie in that domain and that they are decisive), so every output must equal the integer brute force
match_cases.exact_reference in every bit: nn_index, nn_distance, query_idx, train_idx, distance, and for batches n_matched
and match_offsets.  Every comparison is np.array_equal; no tie window is used anywhere."""
import ctypes as C

import numpy as np
import pytest

import match_cases as mc
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.float32 or want.dtype == np.float32:
        eq = _bits(got) == _bits(want)
    else:
        eq = got == want
    if not eq.all():
        bad = np.argwhere(~eq)[:, 0]
        rows = np.unique(bad)[:5]
        raise AssertionError(f"{what}: {np.unique(bad).size} of {got.shape[0]} rows differ, first {rows.tolist()}: "
                             f"got {got[rows].tolist()} want {want[rows].tolist()}")


def _assert_pair(got, ref, what):
    _same(got.nn_index, ref.nn_index, f"{what} nn_index")
    _same(got.nn_distance, ref.nn_distance, f"{what} nn_distance")
    _same(got.query_idx, ref.query_idx, f"{what} query_idx")
    _same(got.train_idx, ref.train_idx, f"{what} train_idx")
    _same(got.distance, ref.distance, f"{what} distance")


def _assert_batch(got, ref, what):
    _assert_pair(got, ref, what)
    _same(got.n_matched, ref.n_matched, f"{what} n_matched")
    _same(got.match_offsets, ref.match_offsets, f"{what} match_offsets")


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_print_split_plan_of_this_device():
    """Which split counts and range lengths the cases reach on the device the tests run on (shown with -s / on failure).
    The expected results do not depend on it: on a partitioned device only this listing differs."""
    cus = _cus()
    print(f"\nsplit plan at {cus} CUs")
    for c in mc.CASES:
        p = mc.split_plan([c.nq], [c.nt], c.D, cus)
        print(f"  {c.name:32s} dp {p.dp:3d} qblocks {p.qblocks:2d} splits {p.splits:2d} tiles/range "
              f"{sorted({e - s for s, e in p.ranges[0]})}")
    for bc in mc.BATCH_CASES:
        p = mc.split_plan([a for a, _ in bc.pairs], [b for _, b in bc.pairs], bc.D, cus)
        empty = [sum(e == s for s, e in r) for r in p.ranges]
        print(f"  {bc.name:32s} dp {p.dp:3d} qblocks {p.qblocks:2d} splits {p.splits:2d} empty ranges per pair {empty}")
    assert cus >= 1


@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_single_pair_cases(name):
    """One-hot k probes, permutations, mass ties, ratio boundaries, planted matches across the compaction tile and the shape
    grid, in the row layouts the case list assigns (contiguous, D + 1 and D + 7 floats per row, NaN or 1e30 in the padding
    columns), at every ratio of the case."""
    case = mc.CASE_BY_NAME[name]
    q, t = mc.arrays(name)
    for layout in case.layouts:
        sq, st = mc.strided(q, layout), mc.strided(t, layout)
        for ratio in case.ratios:
            _assert_pair(api.match_descriptors(sq, st, ratio), mc.reference(name, ratio), f"{name} {layout} ratio {ratio}")


def test_ratio_boundaries_take_the_float_decision():
    """0.3f * 10f rounds to 3f (the exact product is a float midpoint, ties to even): 3 < 3 rejects where a comparison in
    double accepts; equality is not `<`."""
    for rc in mc.RATIO_CASES:
        name = f"ratio_{rc.ratio}_{rc.d0sq}_{rc.d1sq}"
        q, t = mc.arrays(name)
        m = api.match_descriptors(q, t, rc.ratio)
        assert m.query_idx.tolist() == ([0, 1, 2] if rc.accept else []), (name, m.query_idx)
        assert (m.nn_distance == [np.sqrt(np.float32(rc.d0sq)), np.sqrt(np.float32(rc.d1sq))]).all()


@pytest.mark.parametrize("name", [b.name for b in mc.BATCH_CASES])
def test_ragged_batches_at_zero_and_non_zero_first_offsets(name):
    bc = mc.BATCH_BY_NAME[name]
    Q, qo, T, to = mc.batch_arrays(name)
    Qe, qe = mc.embedded(Q, qo, mc.EMBED_Q0)
    Te, te = mc.embedded(T, to, mc.EMBED_T0)
    assert qe[0] == 5 and te[0] == 3
    for ratio in bc.ratios:
        ref = mc.batch_reference(Q, qo, T, to, ratio)
        at0 = api.batch_match_descriptors(mc.strided(Q, bc.layout), qo, mc.strided(T, bc.layout), to, ratio)
        _assert_batch(at0, ref, f"{name} ratio {ratio} offsets from 0")
        emb = api.batch_match_descriptors(mc.strided(Qe, bc.layout), qe, mc.strided(Te, bc.layout), te, ratio)
        _assert_batch(emb, ref, f"{name} ratio {ratio} offsets from 5 / 3")
        for a, b in zip(at0, emb):
            assert np.array_equal(a, b)
        for g, (nq, nt) in enumerate(bc.pairs):          # and each pair on its own
            lo, hi = int(qo[g]), int(qo[g + 1])
            one = api.match_descriptors(Q[lo:hi], T[int(to[g]):int(to[g + 1])], ratio)
            _same(one.nn_index, ref.nn_index[lo:hi], f"{name} pair {g} alone nn_index")
            _same(one.query_idx, ref.query_idx[ref.match_offsets[g]:ref.match_offsets[g + 1]], f"{name} pair {g} alone query_idx")


def test_zero_fill_of_the_packed_rows_does_not_rely_on_a_fresh_allocation():
    """D = 64 with every entry +-8 fills all 64 packed columns; the calls of the same nq / nt at D = 36 and D = 1 that follow
    at once get a workspace of the same size, so stale columns beyond D would show in their scores.  A finite stale query
    column is multiplied by the zero padding of the train rows and vanishes, so the sequence runs a second time after a
    D = 64 call whose queries carry +inf in the upper columns: the packed -inf they leave behind times zero is NaN."""
    nq, nt = 257, 2049
    rng = np.random.default_rng([8, nq, nt])
    for poison in (False, True):
        for D in (64, 36, 1):
            if D == 64:
                q, t = (rng.choice([-8.0, 8.0], size=(n, D)).astype(np.float32) for n in (nq, nt))
            else:
                q, t = (rng.integers(-8, 9, size=(n, D)).astype(np.float32) for n in (nq, nt))
            mc.assert_exact_domain(q, t)
            ref = mc.exact_reference(q, t, 1.0)
            if D == 64 and poison:
                q[:, 1:] = np.inf                      # every query: no neighbours at all (section 3.10, degenerate input)
                none = (np.full((nq, 2), -1, np.int32), np.full((nq, 2), np.inf, np.float32))
                ref = mc.exact_reference(q, t, 1.0, top2=none)
                assert ref.query_idx.size == 0
            _assert_pair(api.match_descriptors(q, t, 1.0), ref, f"D {D} after the D = 64 call{' with inf queries' if poison else ''}")


def _wide(a, pad, fill):
    w = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=np.float32)
    w[:, :a.shape[1]] = a
    return w


@pytest.mark.parametrize("D", [36, 200])
def test_device_entry_point_on_a_callers_stream_with_optional_outputs(D):
    """sba_match_descriptors_device: torch device tensors with rows of D + 7 floats (NaN beyond D), a non-default stream, all
    outputs present and then each one null in turn.  The wanted outputs equal the host entry point's and the reference's;
    the match arrays keep their sentinel beyond n_matched."""
    import torch
    nq, nt, pad, ratio = 257, 2049, 7, 0.5
    q, t = mc.planted_pair(nq, nt, D, 0.5)
    mc.assert_exact_domain(q, t)
    ref = mc.exact_reference(q, t, ratio)
    m = ref.query_idx.size
    assert 0 < m < nq
    wq, wt = _wide(q, pad, np.nan), _wide(t, pad, np.nan)
    host = api.match_descriptors(wq[:, :D], wt[:, :D], ratio)
    _assert_pair(host, ref, "host entry point")
    lib = cabi.load_library()
    dev = torch.device("cuda:0")
    tq, tt = torch.from_numpy(wq).to(dev), torch.from_numpy(wt).to(dev)
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    names = ("nn_index", "nn_dist", "match_q", "match_t", "match_d")
    want = dict(nn_index=host.nn_index, nn_dist=host.nn_distance, match_q=host.query_idx, match_t=host.train_idx,
                match_d=host.distance)
    for missing in ((), ("nn_index",), ("nn_dist",), ("match_q",), ("match_t",), ("match_d",), ("match_q", "match_t", "match_d")):
        out = dict(nn_index=torch.full((nq, 2), -7, dtype=torch.int32, device=dev),
                   nn_dist=torch.full((nq, 2), -7.0, dtype=torch.float32, device=dev),
                   match_q=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                   match_t=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                   match_d=torch.full((nq,), -7.0, dtype=torch.float32, device=dev))
        torch.cuda.synchronize()             # inputs and sentinels are in place before the other stream starts
        ptr = {k: (None if k in missing else C.c_void_p(out[k].data_ptr())) for k in names}
        n = C.c_size_t(12345)
        cabi.check(lib, lib.sba_match_descriptors_device(
            0, C.c_void_p(stream.cuda_stream), C.c_void_p(tq.data_ptr()), nq, C.c_void_p(tt.data_ptr()), nt, D, 4 * (D + pad),
            ratio, ptr["nn_index"], ptr["nn_dist"], C.byref(n), ptr["match_q"], ptr["match_t"], ptr["match_d"]))
        stream.synchronize()
        assert n.value == m, (missing, n.value)
        for k in names:
            got = out[k].cpu().numpy()
            if k in missing:
                assert (got == -7).all(), (missing, k)
            elif k.startswith("nn"):
                _same(got, want[k], f"without {missing}: {k}")
            else:
                _same(got[:m], want[k], f"without {missing}: {k}")
                assert (got[m:] == -7).all(), (missing, k)
    # the inputs were only read
    assert np.array_equal(tq.cpu().numpy(), wq, equal_nan=True) and np.array_equal(tt.cpu().numpy(), wt, equal_nan=True)


def test_nan_train_row_and_inf_query_row_leave_the_other_rows_exact():
    """Section 3.10, degenerate input: a train row with a NaN never ranks, a query with an Inf matches nothing (indices -1,
    distances +inf, never accepted); every other row still equals the integer reference of the remaining rows."""
    nq, nt, D, ratio = 257, 2049, 64, 0.5
    q, t = mc.planted_pair(nq, nt, D, 0.5)
    clean = mc.exact_reference(q, t, ratio)
    bad_q = int(clean.query_idx[3])                    # a query that would be accepted
    bad_t = int(clean.train_idx[10])                   # the nearest row of another accepted query
    assert clean.query_idx[10] != bad_q
    keep = np.flatnonzero(np.arange(nt) != bad_t)
    idx, dist = mc.exact_top2(q, t[keep])
    idx = keep[idx].astype(np.int32)
    idx[bad_q], dist[bad_q] = -1, np.inf
    ref = mc.exact_reference(q, t, ratio, top2=(idx, dist))
    assert bad_q not in ref.query_idx and clean.query_idx[10] not in ref.query_idx and ref.query_idx.size == clean.query_idx.size - 2
    for layout in ("contig", "pad7_nan"):
        sq, st = mc.strided(q, layout), mc.strided(t, layout)
        st[bad_t, D - 1] = np.nan
        sq[bad_q, 0] = np.inf
        got = api.match_descriptors(sq, st, ratio)
        _assert_pair(got, ref, f"NaN train row, Inf query row, {layout}")
        assert (got.nn_index != bad_t).all() and got.nn_index[bad_q].tolist() == [-1, -1] and np.isinf(got.nn_distance[bad_q]).all()


def _keypoints_and_descriptors(sizes, D, seed0):
    """Per pair: key-point records of synthetic.planted_matches (their geometry feeds the evaluation) with planted integer
    descriptors of this file's own; about half the left rows find their right row at ratio 0.5."""
    pms = [synthetic.planted_matches(n, dl, dr, seed=seed0 + i) for i, (n, dl, dr) in enumerate(sizes)]
    descs = [mc.planted_pair(p.left_kp.shape[0], p.right_kp.shape[0], D, 0.5) if p.right_kp.shape[0] else
             (mc.random_pair("upload", p.left_kp.shape[0], 0, D)) for p in pms]
    return pms, descs


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32])
def test_problem_upload_matches_on_integer_descriptors(store):
    (pm,), ((dl, dr),) = _keypoints_and_descriptors([(2000, 150, 400)], 36, 31)
    ratio = 0.5
    ref = mc.exact_reference(dl, dr, ratio)
    assert mc.compact_tile() < dl.shape[0] and 0 < ref.query_idx.size < dl.shape[0]
    kl, kr = pm.left_kp[ref.query_idx], pm.right_kp[ref.train_idx]
    rot, tran = pm.geometry.rot_init, pm.geometry.tran_init
    for depth in (None, 6.0):
        d12 = None if depth is None else np.full((kl.shape[0], 2), depth)
        with api.Problem(0) as a, api.Problem(0) as b:
            ml, mr = a.upload_matches(pm.left_kp, pm.right_kp, mc.strided(dl, "pad7_nan"), mc.strided(dr, "pad7_nan"),
                                      pm.im_width, pm.im_height, ratio=ratio, init_depth=depth, store=store)
            _same(ml, ref.query_idx, "match_left")
            _same(mr, ref.train_idx, "match_right")
            b.upload_keypoints(kl, kr, pm.im_width, pm.im_height, d12=d12, store=store)
            assert a.size == b.size == ref.query_idx.size
            dms = [api.DEPTH_UNIFORM] + ([api.DEPTH_PER_MATCH] if depth is not None else [])
            for mode in (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT):
                for dm in dms:
                    pa = a.eval_pack(mode, rot, tran, 5.0, 7.0, depth_mode=dm)
                    pb = b.eval_pack(mode, rot, tran, 5.0, 7.0, depth_mode=dm)
                    assert np.array_equal(pa, pb), (mode, dm)


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32])
def test_batch_upload_matches_at_non_zero_first_offsets(store):
    sizes = [(600, 100, 300), (0, 30, 50), (300, 0, 0), (0, 0, 0), (0, 40, 0), (500, 200, 100), (0, 1, 1)]
    pms, descs = _keypoints_and_descriptors(sizes, 36, 40)
    B, ratio = len(pms), 0.5
    lo = np.concatenate([[0], np.cumsum([p.left_kp.shape[0] for p in pms])]).astype(np.uint64)
    ro = np.concatenate([[0], np.cumsum([p.right_kp.shape[0] for p in pms])]).astype(np.uint64)
    KL = np.concatenate([p.left_kp for p in pms]); KR = np.concatenate([p.right_kp for p in pms])
    DL = np.concatenate([d[0] for d in descs]); DR = np.concatenate([d[1] for d in descs])
    W, H = pms[0].im_width, pms[0].im_height
    ref = mc.batch_reference(DL, lo, DR, ro, ratio)
    assert (ref.n_matched > 0).sum() >= 3 and (ref.n_matched == 0).sum() >= 3
    # rows 5 / 3 before the first pair and 4 after the last one hold NaN: key-point records and descriptors alike
    KLe, loe = mc.embedded(KL, lo, mc.EMBED_Q0); KRe, roe = mc.embedded(KR, ro, mc.EMBED_T0)
    DLe, _ = mc.embedded(DL, lo, mc.EMBED_Q0); DRe, _ = mc.embedded(DR, ro, mc.EMBED_T0)
    assert loe[0] == 5 and roe[0] == 3
    depths = np.arange(4.0, 4.0 + B)
    x1, x2, d12 = [], [], []
    for g, p in enumerate(pms):
        s = slice(int(ref.match_offsets[g]), int(ref.match_offsets[g + 1]))
        x1.append(api.keypoints_to_sphere(p.left_kp[ref.query_idx[s]], W, H).reshape(-1, 3))
        x2.append(api.keypoints_to_sphere(p.right_kp[ref.train_idx[s]], W, H).reshape(-1, 3))
        d12.append(np.full((s.stop - s.start, 2), depths[g]))
    off = ref.match_offsets.astype(np.uint64)
    rot = np.stack([p.geometry.rot_init for p in pms]); tran = np.stack([p.geometry.tran_init for p in pms])
    for depth in (None, depths):
        with api.Batch(0) as a, api.Batch(0) as a0, api.Batch(0) as b:
            ml, mr, n = a.upload_matches(KLe, loe, KRe, roe, mc.strided(DLe, "pad1_big"), mc.strided(DRe, "pad1_big"), W, H,
                                         ratio=ratio, init_depth=depth, store=store)
            _same(ml, ref.query_idx, "match_left")
            _same(mr, ref.train_idx, "match_right")
            _same(n, ref.n_matched, "n_matched")
            ml0, mr0, n0 = a0.upload_matches(KL, lo, KR, ro, DL, DR, W, H, ratio=ratio, init_depth=depth, store=store)
            assert np.array_equal(ml0, ml) and np.array_equal(mr0, mr) and np.array_equal(n0, n)
            b.upload(np.concatenate(x1), np.concatenate(x2), off, None if depth is None else np.concatenate(d12), store=store)
            assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a0.offsets, b.offsets)
            dms = [api.DEPTH_UNIFORM] + ([api.DEPTH_PER_MATCH] if depth is not None else [])
            for mode in (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT):
                for dm in dms:
                    pb = b.eval(mode, rot, tran, np.full(B, 5.0), np.full(B, 7.0), depth_mode=dm)
                    for h in (a, a0):
                        assert np.array_equal(h.eval(mode, rot, tran, np.full(B, 5.0), np.full(B, 7.0), depth_mode=dm), pb), (mode, dm)
