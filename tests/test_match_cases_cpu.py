"""CPU: the integer descriptor cases of tests/match_cases.py on their own -- what keeps tests/test_gpu_match_exact.py from
being vacuous.  Every case lies in the domain where the device arithmetic is exact; the exact reference agrees with a plain
Python loop; the cases are decisive (a dropped component, a dropped train row, a wrong tie order changes the expected
output); and the case list reaches the split counts, range lengths and block boundaries of the documented split rule at
256 CUs.  No product code runs here."""
import numpy as np
import pytest

import match_cases as mc

CUS = 256


def test_every_case_is_in_the_exact_domain():
    for case in mc.CASES:
        q, t = mc.arrays(case.name)
        assert q.shape == (case.nq, case.D) and t.shape == (case.nt, case.D) and q.dtype == t.dtype == np.float32, case.name
        mc.assert_exact_domain(q, t)
        assert case.layouts
        for layout in case.layouts:
            sq, st = mc.strided(q, layout), mc.strided(t, layout)
            assert np.array_equal(sq, q) and np.array_equal(st, t)
            pad, fill = mc.LAYOUTS[layout]
            assert st.strides == (4 * (case.D + pad), 4)
            if pad:
                wide = np.lib.stride_tricks.as_strided(st, (case.nt, case.D + pad), st.strides)
                assert np.array_equal(wide[:, case.D:], np.full((case.nt, pad), fill, np.float32), equal_nan=True)
    for bc in mc.BATCH_CASES:
        Q, qo, T, to = mc.batch_arrays(bc.name)
        mc.assert_exact_domain(Q, T)
        assert [int(b - a) for a, b in zip(qo[:-1], qo[1:])] == [p[0] for p in bc.pairs]
        assert [int(b - a) for a, b in zip(to[:-1], to[1:])] == [p[1] for p in bc.pairs]
    with pytest.raises(AssertionError):
        mc.assert_exact_domain(np.full((1, 256), 148, np.float32), np.zeros((1, 256), np.float32))
    mc.assert_exact_domain(np.full((1, 256), 147, np.float32), np.zeros((1, 256), np.float32))
    with pytest.raises(AssertionError):
        mc.assert_exact_domain(np.full((1, 4), 0.5, np.float32), np.zeros((1, 4), np.float32))


def _loop_reference(q, t, ratio):
    """Independent of exact_reference: Python integers, a sort of (d^2, index) tuples per query, math.sqrt rounded once."""
    import math
    nn_i, nn_d, acc = [], [], []
    for i in range(len(q)):
        cand = sorted((sum((int(a) - int(b)) ** 2 for a, b in zip(q[i], t[j])), j) for j in range(len(t)))[:2]
        idx = [c[1] for c in cand] + [-1] * (2 - len(cand))
        # sqrt of an integer below 2^24 in double, rounded to float32: no double rounding for a 24-bit argument
        d = [np.float32(math.sqrt(c[0])) for c in cand] + [np.float32(np.inf)] * (2 - len(cand))
        nn_i.append(idx)
        nn_d.append(d)
        if len(cand) == 2 and d[0] < np.float32(np.float32(ratio) * d[1]):
            acc.append(i)
    return np.array(nn_i, np.int32).reshape(-1, 2), np.array(nn_d, np.float32).reshape(-1, 2), np.array(acc, np.int32)


@pytest.mark.parametrize("name,ratio", [("ties_small_257x513_D5", 0.9), ("grid_D2_256x129", 1.0), ("onehot_D5", 1.5),
                                        ("ratio_0.3_9_100", 0.3)])
def test_exact_reference_against_a_python_loop(name, ratio):
    q, t = mc.arrays(name)
    q = q[:40]
    ref = mc.exact_reference(q, t, ratio)
    nn_i, nn_d, acc = _loop_reference(q, t, ratio)
    assert np.array_equal(ref.nn_index, nn_i) and np.array_equal(ref.nn_distance.view(np.uint32), nn_d.view(np.uint32))
    assert np.array_equal(ref.query_idx, acc) and np.array_equal(ref.train_idx, nn_i[acc, 0])
    assert np.array_equal(ref.distance, nn_d[acc, 0])
    # the literal int64 sum of squared differences
    d2 = ((q.astype(np.int64)[:, None, :] - t.astype(np.int64)[None, :, :]) ** 2).sum(2)
    assert np.array_equal(mc.squared_distances(q, t), d2)


def test_reference_with_fewer_than_two_train_rows_and_batches():
    q = np.array([[1, 2], [3, 4]], np.float32)
    r = mc.exact_reference(q, q[:1], 1.5)
    assert r.nn_index.tolist() == [[0, -1], [0, -1]] and r.query_idx.size == 0
    assert r.nn_distance[0].tolist() == [0.0, np.inf] and r.nn_distance[1, 0] == np.sqrt(np.float32(8))
    r = mc.exact_reference(q, q[:0], 1.5)
    assert r.nn_index.tolist() == [[-1, -1]] * 2 and np.isinf(r.nn_distance).all() and r.query_idx.size == 0
    assert mc.exact_reference(q[:0], q, 0.3).nn_index.shape == (0, 2)
    for bc in mc.BATCH_CASES:
        Q, qo, T, to = mc.batch_arrays(bc.name)
        b = mc.batch_reference(Q, qo, T, to, bc.ratios[0])
        assert b.nn_index.shape == (Q.shape[0], 2) and b.match_offsets[-1] == b.query_idx.size == b.n_matched.sum()
        assert np.array_equal(np.diff(b.match_offsets), b.n_matched)
        nonempty = [g for g, (nq, nt) in enumerate(bc.pairs) if nq > 1 and nt > 1]
        assert all(b.n_matched[g] > 0 for g in nonempty if bc.ratios[0] >= 0.3), b.n_matched
        assert (b.n_matched < np.array([p[0] for p in bc.pairs]))[nonempty].any()      # the compaction drops something
        for g, (nq, nt) in enumerate(bc.pairs):
            if nt < 2:
                assert b.n_matched[g] == 0
        # embedding moves the offsets and nothing else
        Qe, qe = mc.embedded(Q, qo, mc.EMBED_Q0)
        Te, te = mc.embedded(T, to, mc.EMBED_T0)
        assert qe[0] == 5 and te[0] == 3 and np.isnan(Qe[:5]).all() and np.isnan(Qe[int(qe[-1]):]).all() and np.isnan(Te[:3]).all()
        e = mc.batch_reference(Qe, qe, Te, te, bc.ratios[0])
        assert all(np.array_equal(x, y) for x, y in zip(b, e))


# -- mutation checks ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", mc.ALL_D)
def test_onehot_every_k_is_decisive(D):
    """Component k dropped from the product (= zeroed on the query side) changes nn_index of query k.  With D = 1 the one-hot
    case has two train rows only and cannot show it; there the D = 1 cases of the shape grid do (nt > 2, 17 distinct
    values: without the product every query would get the rows of smallest |t|)."""
    q, t = mc.arrays(f"onehot_D{D}")
    idx, dist = mc.top2(f"onehot_D{D}")
    k = np.arange(D)
    assert np.array_equal(idx[:, 0], np.minimum(k, 2 * D - 1 - k)) and np.array_equal(idx[:, 1], np.maximum(k, 2 * D - 1 - k))
    assert (dist == 0).all()
    d2 = mc.squared_distances(q, t)
    d2[k, idx[:, 0]] = d2[k, idx[:, 1]] = 8
    assert (d2 == 8).all()                        # everything else sits at 8
    if D == 1:
        grid = [c for c in mc.CASES if c.family == "grid" and c.D == 1 and c.nt > 2]
        assert grid
        for c in grid:
            gq, gt = mc.arrays(c.name)
            assert (mc.exact_top2(np.zeros_like(gq), gt)[0] != mc.top2(c.name)[0]).any(), c.name
        return
    for kk in range(D):
        mq = q[kk:kk + 1].copy()
        mq[0, kk] = 0
        assert (mc.exact_top2(mq, t)[0] != idx[kk]).any(), kk
        # the train side: rows k and 2 D - 1 - k no longer stand out against a query that still carries component k ...
        mt = t.copy()
        mt[:, kk] = 0
        got = mc.exact_top2(q[kk:kk + 1], mt)
        # ... they stay nearest (4 against 8) but the distances change, which the bitwise nn_distance check sees
        assert (got[1] != dist[kk]).any(), kk


@pytest.mark.parametrize("name", [c.name for c in mc.CASES if c.family == "perm"])
def test_permutation_every_train_row_is_decisive(name):
    case = mc.CASE_BY_NAME[name]
    q, t = mc.arrays(name)
    idx, dist = mc.top2(name)
    pi = mc.perm_of(case.nq, case.nt, case.D)
    assert np.array_equal(idx[:, 0], pi) and (dist[:, 0] == 0).all()
    assert np.unique(pi).size == case.nq                       # each touched train row is the top-1 of exactly one query
    assert (dist[:, 1] > 0).all()                              # and the only row at 0: without it the answer changes
    assert (dist[:, 1] ** 2 >= 100).all(), dist[:, 1].min()    # the second neighbour is far away
    if case.nq == case.nt:
        assert np.array_equal(np.sort(pi), np.arange(case.nt))   # every train row
    else:
        # one row in every tile, all 32 positions of a tile, both lane halves, every split range of the 256-CU plan
        assert np.unique(pi // mc.TRAIN_TILE).size == case.nq and np.unique(pi % mc.TRAIN_TILE).size == mc.TRAIN_TILE
        plan = mc.split_plan([case.nq], [case.nt], case.D, CUS)
        assert plan.splits == 64 and np.unique(mc.range_of(plan, 0, pi)).size == 64
    if case.nt <= 129:                                         # the literal deletion
        for r in range(case.nt):
            keep = np.arange(case.nt) != r
            got = mc.exact_top2(q, t[keep])[0]
            back = np.flatnonzero(keep)[got]                   # indices of the full train set
            assert (back != idx).any(), r


def _tie_stats(name):
    q, t = mc.arrays(name)
    d2 = np.sort(mc.squared_distances(q, t), axis=1)
    return (d2[:, 0] == d2[:, 1]).mean(), (d2[:, 1] == d2[:, 2]).mean()


def test_mass_ties_are_frequent_and_spread():
    for c in mc.CASES:
        if c.family == "ties_small":
            t12, t23 = _tie_stats(c.name)
            assert t12 >= 0.15 and t23 >= 0.15, (c.name, t12, t23)
        if c.family != "ties_pool":
            continue
        t12, _ = _tie_stats(c.name)
        assert t12 >= 0.80, (c.name, t12)
        idx, dist = mc.top2(c.name)
        tied = dist[:, 0] == dist[:, 1]
        i0, i1 = idx[tied, 0].astype(np.int64), idx[tied, 1].astype(np.int64)
        assert (i0 < i1).all()                                  # the lower index first
        half0, half1 = (i0 % 8) < 4, (i1 % 8) < 4
        assert (half0 & ~half1).any() and (~half0 & half1).any() and (half0 & half1).any() and (~half0 & ~half1).any()
        tile0, tile1 = i0 // mc.TRAIN_TILE, i1 // mc.TRAIN_TILE
        assert (tile0 != tile1).any()
        plan = mc.split_plan([c.nq], [c.nt], c.D, CUS)
        assert plan.splits > 1
        r0, r1 = mc.range_of(plan, 0, i0), mc.range_of(plan, 0, i1)
        assert (r0 != r1).any() and ((r0 == r1) & (tile0 != tile1)).any(), c.name
    # copies that meet inside one lane (same tile, same half), inside one wave (same tile, other half), across tiles of one
    # range and across ranges: all four merge levels see a tie in the largest pool case
    idx, dist = mc.top2("ties_pool_257x2049_D64")
    tied = dist[:, 0] == dist[:, 1]
    i0, i1 = idx[tied, 0].astype(np.int64), idx[tied, 1].astype(np.int64)
    same_tile = i0 // 32 == i1 // 32
    assert (same_tile & ((i0 % 8 < 4) == (i1 % 8 < 4))).any() and (same_tile & ((i0 % 8 < 4) != (i1 % 8 < 4))).any()


def test_planted_cases_cross_the_compaction_tile():
    tile = mc.compact_tile()
    assert tile % 256 == 0 and tile >= 256
    for c in mc.CASES:
        if c.family != "planted":
            continue
        assert c.nq > tile
        for ratio in c.ratios:
            ref = mc.reference(c.name, ratio)
            share = ref.query_idx.size / c.nq
            if c.name.endswith("_all"):
                assert share == 1.0, (c.name, share)
            else:
                assert 0.25 <= share <= 0.40, (c.name, share)
            assert (ref.query_idx < tile).any() and (ref.query_idx >= tile).any()
            assert set(np.unique(ref.distance ** 2).round().tolist()) <= {1.0, 2.0} and (ref.nn_distance[ref.query_idx, 1] > 10).all()
    assert any(c.nq > 2 * tile for c in mc.CASES if c.family == "planted")


def test_random_cases_accept_at_some_ratio_and_not_everything():
    """The ratios 0.3 / 0.9 / 1.0 of the random families: at 1.0 most queries pass unless they tie, at 0.3 next to none."""
    some = 0
    for c in mc.CASES:
        if c.family not in ("grid", "ties_small", "ties_pool", "perm") or c.nt < 2:
            continue
        n10 = mc.reference(c.name, 1.0).query_idx.size
        n03 = mc.reference(c.name, 0.3).query_idx.size
        assert n03 <= n10 <= c.nq
        some += 0 < n10 < c.nq
    assert some >= 20


# -- coverage of the split rule at 256 CUs ----------------------------------------------------------------------------------

def test_split_plan_restates_the_rule():
    p = mc.split_plan([2000], [2000], 64, 256)       # 8 query blocks -> 128 wanted, 63 tiles allow 15
    assert (p.dp, p.query_block, p.qblocks, p.splits) == (64, 256, 8, 15)
    assert p.ranges[0][0] == (0, 4) and p.ranges[0][-1] == (58, 63) and len(p.ranges[0]) == 15
    assert mc.split_plan([50000], [50000], 64, 256).splits == 6          # 196 blocks -> ceil(1024 / 196)
    assert mc.split_plan([1], [8193], 256, 256).splits == 64 and mc.split_plan([1], [8193], 256, 256).query_block == 128
    assert mc.split_plan([300000], [8193], 64, 256).splits == 1
    assert mc.split_plan([1], [224], 64, 256).splits == 1 and mc.split_plan([1], [256], 64, 256).splits == 2
    assert mc.split_plan([1], [8193], 64, 8).splits == 32
    b = mc.split_plan([1, 0, 5], [70, 10, 3000], 36, 256)
    assert b.qblocks == 2 and b.splits == 23 and [len(r) for r in b.ranges] == [23, 23, 23]
    assert sum(e > s for s, e in b.ranges[0]) == 3 and all(e - s <= 1 for s, e in b.ranges[0])
    for rs, tiles in zip(b.ranges, (3, 1, 94)):      # the ranges tile [0, tiles) in order
        assert rs[0][0] == 0 and rs[-1][1] == tiles and all(a[1] == b_[0] for a, b_ in zip(rs[:-1], rs[1:]))


def test_case_list_covers_the_split_rule():
    plans = {c.name: mc.split_plan([c.nq], [c.nt], c.D, CUS) for c in mc.CASES}
    splits = {p.splits for p in plans.values()}
    assert 1 in splits and 64 in splits and any(1 < s < 64 for s in splits)
    lengths = lambda p: {e - s for s, e in p.ranges[0]}
    assert any(len(lengths(p)) > 1 for p in plans.values())                       # unequal ranges within one call
    every = set().union(*(lengths(p) for p in plans.values() if p.splits > 1))
    assert any(n % 2 for n in every) and any(n % 2 == 0 and n > 0 for n in every)
    for bc in mc.BATCH_CASES[:2]:
        p = mc.split_plan([a for a, _ in bc.pairs], [b for _, b in bc.pairs], bc.D, CUS)
        assert p.splits > 1
        tiles = [-(-nt // mc.TRAIN_TILE) for _, nt in bc.pairs]
        assert any(0 < T < p.splits and nq > 0 for T, (nq, _) in zip(tiles, bc.pairs))         # a pair with empty ranges
    for dp in (64, 128, 256):
        mine = [c for c in mc.CASES if c.family == "grid" and mc.padded_dim(c.D) == dp]
        qb = mc.query_block(mine[0].D)
        for nt in (33, 2049, 8193):
            assert {1, qb - 1, qb, qb + 1} <= {c.nq for c in mine if c.nt == nt}, (dp, nt)


def test_shape_grid_and_layout_coverage():
    grid = [c for c in mc.CASES if c.family == "grid"]
    assert len(grid) <= 60 and len({(c.D, c.nq, c.nt) for c in grid}) == len(grid)
    assert {c.D for c in grid} == set(mc.ALL_D) and {c.nq for c in grid} == set(mc.ALL_NQ) and {c.nt for c in grid} == set(mc.ALL_NT)
    assert {c.D for c in mc.CASES if c.family == "onehot"} == set(mc.ALL_D)
    assert max(max(c.nq, c.nt) for c in mc.CASES) <= 8193 and max(c.D for c in mc.CASES) <= 256
    for family in {c.family for c in mc.CASES}:
        layouts = {l for c in mc.CASES if c.family == family for l in c.layouts}
        pads = {mc.LAYOUTS[l][0] for l in layouts}
        fills = {"nan" if np.isnan(mc.LAYOUTS[l][1]) else "big" for l in layouts if mc.LAYOUTS[l][0]}
        assert pads == {0, 1, 7} and fills == {"nan", "big"}, (family, layouts)
    assert any(c.D % 4 and c.layouts != ("contig",) for c in grid)      # 16-byte reads that straddle D, next to NaN columns
    assert {"contig"} < {bc.layout for bc in mc.BATCH_CASES}
    for bc in mc.BATCH_CASES:
        assert len(bc.pairs) >= 7
        assert {(0, 0)} < set(bc.pairs) and any(nq == 0 < nt for nq, nt in bc.pairs) and any(nt == 0 < nq for nq, nt in bc.pairs)
        assert any(nt == 1 for _, nt in bc.pairs) and any(nq == 1 for nq, _ in bc.pairs)


# -- the ratio boundaries ---------------------------------------------------------------------------------------------------

def test_ratio_boundaries_float32_against_float64():
    assert np.float32(0.3) * np.float32(10) == np.float32(3) and float(np.float32(0.3)) * 10.0 > 3.0     # the midpoint, to even
    differ = 0
    for rc in mc.RATIO_CASES:
        name = f"ratio_{rc.ratio}_{rc.d0sq}_{rc.d1sq}"
        ref = mc.reference(name, rc.ratio)
        idx, dist = mc.top2(name)
        assert (dist[:, 0] == np.sqrt(np.float32(rc.d0sq))).all() and (dist[:, 1] == np.sqrt(np.float32(rc.d1sq))).all()
        assert (idx[:, 0] != idx[:, 1]).all() and (rc.d0sq != rc.d1sq or (idx[:, 0] < idx[:, 1]).all())
        assert ref.query_idx.tolist() == ([0, 1, 2] if rc.accept else []), name
        f64 = np.sqrt(float(rc.d0sq)) < float(np.float32(rc.ratio)) * np.sqrt(float(rc.d1sq))
        assert f64 == rc.accept_f64, name
        differ += f64 != rc.accept
    assert differ == 2
