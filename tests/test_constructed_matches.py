"""The constructed matcher families (tests/constructed_matches.py) without a GPU: the constants they are shaped around are the ones in
the sources, every family's stated facts hold against the contracts (tests/numpy_matches.py, tests/numpy_affine.py), and each family
tells the contract from a plausibly wrong variant.

The variants are restatements with ONE mistake each, of the kind the four kernels can carry unnoticed; they live in the constructed
module, are numpy only and are never imported by the product:

  variant                                                          family that tells it from the contract
  the running pair (d1, d2) reset at each tile                     M1 tiles (every query image against every train image)
  the last, partial tile compared over all 256 slots               M1 tiles (257, 513, 600: a planted neighbour in slot 255 or 511)
  the float test d1 < (1 - match_conf) d2                          M2 ratio edges, at (7, 10) and (70, 100)
  <= in the ratio test                                             M2 ratio edges: (0, 0) at every T; (d, d), (256, 256) at T = 1024
  the duplicate test without nn_matched(f, T)                      M3 placements "none" (the X rows, the first of each tied pair)
  the duplicate test applied without a forward direction           M3 pair shapes, pair (0, 1)
  a wavefront's `before` counted with w <= wave                    M3 placements (all four)
  < in match_inlier                                                M4 threshold, all three models
  >= in match_pick's loop                                          M5 hypothesis ties, all three models, from 300 iterations
  the tree without its k term | the largest k among equals         M5 hypothesis ties, all three models, every iteration count
  the sampler keyed by the pair's position in the table            M6 many pairs
Nothing here provokes a fault: these are host computations."""
import os
import re

import numpy as np
import pytest

from tests import constructed_matches as CM
from tests import numpy_affine as NA
from tests import numpy_matches as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stitching_amd", "csrc")


def _src(name, where=CSRC):
    return open(os.path.join(where, name)).read()


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1), 0)


def test_the_kernels_constants_are_the_ones_the_families_are_shaped_around():
    hdr, hip, host = _src("stx_internal.h"), _src("stx_matches.hip"), _src("stx_matches_host.cpp")
    assert CM.NN_WG == _int(r"constexpr\s+int\s+STX_MATCH_NN_WG\s*=\s*(\d+)\s*;", hdr)
    assert CM.HYP_PER_WG == _int(r"constexpr\s+int\s+STX_MATCH_HYP_PER_WG\s*=\s*(\d+)\s*;", hdr)
    assert CM.NO_D == _int(r"constexpr\s+unsigned\s+STX_MATCH_NO_D\s*=\s*(0x[0-9a-fA-F]+)u\s*;", hdr) == NM.NO_D2
    # match_2nn: one tile of STX_MATCH_NN_WG train descriptors at a time, strict < on an ascending scan
    assert re.search(r"for \(int t0 = 0; t0 < J\.nb; t0 \+= STX_MATCH_NN_WG\)", hip) and re.search(r"const int cnt = min\(STX_MATCH_NN_WG, J\.nb - t0\);", hip)
    assert re.search(r"if \(d < d1\) \{ d2 = d1; d1 = d; i1 = \(unsigned\)\(t0 \+ t\); \}\s*else if \(d < d2\) d2 = d;", hip)
    assert re.search(r"const int q = \(\(int\)blockIdx\.x - J\.block0\) \* STX_MATCH_NN_WG \+ tid;", hip)
    # match_union: chunks of 256 in both passes, four wavefronts in block_place, the integer ratio rule, the guarded duplicate test
    assert CM.UNION_CHUNK == _int(r"for \(int q0 = 0; q0 < P\.ni; q0 \+= (\d+)\)", hip) == _int(r"for \(int t0 = 0; t0 < P\.nj; t0 \+= (\d+)\)", hip)
    assert CM.UNION_CHUNK == _int(r"__launch_bounds__\((\d+)\) void match_union_kernel", hip) == 64 * _int(r"for \(int w = 0; w < (\d+); w\+\+\)", hip)
    assert re.search(r"if \(w < wave\) before \+= c;", hip)
    assert re.search(r"return 1024u \* \(e\.y & 0xffffu\) < T \* \(e\.y >> 16\);", hip)
    assert re.search(r"if \(flag && P\.nn_f >= 0\) \{", hip) and re.search(r"if \(nn_matched\(f, T\) && \(int\)f\.x == t\) flag = false;", hip)
    # match_ransac and match_pick: nothing below 6 matches; hypotheses tid, tid + 256, ...; the tree over 256 threads
    assert hip.count("if (m < %d)" % CM.MIN_MATCHES) == 2 and len(re.findall(r"if \(m < (\d+)\)", hip)) == 2
    assert CM.MIN_MATCHES == NM.MIN_MATCHES == _int(r"MIN_MATCHES = (\d+)", _src("match_estimation.py", os.path.join(ROOT, "stitching_amd")))
    assert CM.PICK_WG == _int(r"for \(int k = tid; k < iters; k \+= (\d+)\) \{", hip) == _int(r"__shared__ int s_n\[(\d+)\], s_k\[\d+\];", hip)
    assert CM.PICK_WG == 2 * _int(r"for \(int o = (\d+); o; o >>= 1\) \{", hip) == _int(r"__launch_bounds__\((\d+)\) void match_pick_kernel", hip)
    assert re.search(r"if \(n > best\) \{ best = n; bk = k; \}", hip)
    assert re.search(r"if \(n > s_n\[tid\] \|\| \(n == s_n\[tid\] && k < s_k\[tid\]\)\)", hip)
    assert re.search(r"<= __dmul_rn\(t2, __dmul_rn\(W, W\)\);", hip)
    assert re.search(r"const int k = \(int\)\(blockIdx\.x % \(unsigned\)hb\) \* STX_MATCH_HYP_PER_WG \+ \(threadIdx\.x >> 6\);", hip)
    # the host's tables
    assert CM.MIN_TRAIN == _int(r"if \(na == 0 \|\| nb < (\d+)\) return -1;", host)
    assert re.search(r"P\.p = \(int\)\(\(unsigned\)i \* \(unsigned\)n \+ \(unsigned\)j\);", host)
    assert CM.T_DEFAULT == NM.ratio_threshold(0.3) and [NM.ratio_threshold(c) for c in CM.RATIO_CONFS] == [717, 1024, 0]
    # the shapes lie around them
    assert set(CM.TILE_TRAINS) == {CM.NN_WG + 1, 2 * CM.NN_WG, 2 * CM.NN_WG + 1, 600} and set(CM.TILE_QUERIES) == {1, CM.NN_WG, CM.NN_WG + 1}
    assert CM.tile_slots(600) == [0, 255, 256, 511, 512, 599] and CM.tile_slots(257) == [0, 255, 256] and CM.tile_slots(512) == [0, 255, 256, 511]
    assert set(CM.TIES_ITERS) == {CM.PICK_WG - 1, CM.PICK_WG, CM.PICK_WG + 1, 300, 4096}
    assert set(CM.SEVEN) == {63, 64, CM.UNION_CHUNK - 1, CM.UNION_CHUNK, 2 * CM.UNION_CHUNK - 1, 2 * CM.UNION_CHUNK, CM.NQ - 1}
    f = CM.built("many_pairs").facts
    assert f["hb"] == 2 and f["last_block_live"] == 3 and CM.MANY_ITERS == 7


def _pair_descs(case, i, j):
    return case.features[i]["descriptors"], case.features[j]["descriptors"]


# ---- M1 ----------------------------------------------------------------------------------------------------------------------------------
def test_tiles():
    case = CM.built("tiles")
    f = case.facts
    CM.assert_rows(case, CM.contract("homography", "tiles"))
    for (qi, ti), rows in f["rows"].items():
        nq, nb = len(case.features[qi]["x"]), len(case.features[ti]["x"])
        slots = CM.tile_slots(nb)
        A, B = _pair_descs(case, qi, ti)
        assert CM.forward_rows(A, B, CM.T_DEFAULT) == rows
        if nq > 1:  # every ordered pair of slots has a query of its own; two workgroups have planted queries at 255 and 256
            assert f["slot_pairs"][(nq, nb)] == [(a, b) for a in slots for b in slots if a != b]
            assert {r[0] for r in rows} >= {0, 255} and (nq == CM.NN_WG or 256 in {r[0] for r in rows})
            assert {p for p, _, _ in CM.tile_positions(nq)} >= {0, 63, 64, 127, 128, 191, 255}
            assert sorted({r[1] for r in rows}) == slots
        else:
            assert rows == [(0, 255, 4)]
        # the variants
        assert CM.forward_rows(A, B, CM.T_DEFAULT, CM.two_nn_reset) != rows
        stale = CM.forward_rows(A, B, CM.T_DEFAULT, CM.two_nn_stale)
        # the stale slots of 257 are tile 0's 1 .. 255, of 513 tile 1's 1 .. 255, of 600 tile 1's 88 .. 255: slot 255 or 511 comes twice
        assert (stale == rows) == (nb % CM.NN_WG == 0 or (nq == 1 and nb != 257)), (nq, nb)
    assert {nb for _, nb in f["slot_pairs"]} == set(CM.TILE_TRAINS)


# ---- M2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conf", CM.RATIO_CONFS)
def test_ratio_edges(conf):
    case = CM.built("ratio_edges", conf)
    f = case.facts
    CM.assert_rows(case, CM.contract("homography", "ratio_edges", conf))
    got = dict(zip(f["pairs"], f["matched"]))
    if conf == 0.3:
        assert [p for p in f["pairs"] if got[p]] == [(0, 1), (7, 10), (70, 100), (1, 2)]
        # the float restatement differs at (7, 10), and at its tenfold: 0.7 * 10 rounds to 7.0
        assert [p for p in f["pairs"] if CM.ratio_float(*p, conf) != got[p]] == [(7, 10), (70, 100)]
    elif conf == 0.0:
        assert got[(255, 256)] and not got[(256, 256)] and not got[(5, 5)] and got[(71, 101)]
    else:
        assert not any(f["matched"])
    le = [p for p in f["pairs"] if CM.ratio_le(*p, f["T"]) != got[p]]  # equality 1024 d1 == T d2: 0 == 0 at every T, d == d at T = 1024
    assert le == {0.3: [(0, 0)], 0.0: [(1, 1), (5, 5), (0, 0), (256, 256)], 1.0: [(0, 1), (0, 0)]}[conf]
    for (i, j), rows in f["rows"].items():  # each distance pair is exactly what the builder says
        q, t = (i, j) if i % 2 == 0 else (j, i)
        d = np.sort(CM.hamming(*_pair_descs(case, q, t))[0])
        assert tuple(d.tolist()) == f["pairs"][min(i, j) // 2]


# ---- M3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CM.PLACEMENTS)
def test_placements(which):
    case = CM.built("placements", which)
    f = case.facts
    want = CM.contract("homography", "placements", which)
    CM.assert_rows(case, want)
    rows = f["rows"][(0, 1)]
    assert len(rows) == {"seven": 7, "hole": 344, "all": 640, "none": 224}[which] and f["forward"] == {"seven": 7, "hole": 344, "all": 600, "none": 0}[which]
    fwd = [r[0] for r in rows[:f["forward"]]]
    if which == "seven":
        assert fwd == list(CM.SEVEN)
    if which == "hole":
        assert fwd == [q for q in range(CM.NQ) if not CM.UNION_CHUNK <= q < 2 * CM.UNION_CHUNK]
    if which in ("all", "none"):
        back = rows[f["forward"]:]
        assert [r[1] for r in back] == sorted(r[1] for r in back) and back[0][1] >= CM.UNION_CHUNK and back[-1][1] >= 2 * CM.UNION_CHUNK
    A, B = _pair_descs(case, 0, 1)
    assert CM.union_variant(A, B, CM.T_DEFAULT, "contract").tolist() == [list(r) for r in rows]
    assert CM.union_variant(A, B, CM.T_DEFAULT, "before_le").tolist() != [list(r) for r in rows]
    without = CM.union_variant(A, B, CM.T_DEFAULT, "dup_without_ratio")
    if which == "none":  # the X rows: their queries' nearest neighbour is X itself, by a forward match that failed the ratio test
        i1, d1, d2 = NM.two_nn(A, B)
        assert len(f["kept_same_t"]) == 12 and all(i1[q] == t and (d1[q], d2[q]) == (3, 4) for q, t, _ in f["kept_same_t"])
        kept = {tuple(r) for r in without.tolist()}
        # and the first of every pair A, B, which a forward tie names as the nearest
        assert len(without) == len(rows) - 12 - 100 and not kept & set(f["kept_same_t"])
    else:
        assert without.tolist() == [list(r) for r in rows]


def test_pair_shapes():
    case = CM.built("pair_shapes")
    want = CM.contract("homography", "pair_shapes")
    CM.assert_rows(case, want)
    assert [len(f["x"]) for f in case.features] == [3, 1, 1, 3]
    A, B = _pair_descs(case, 0, 1)
    assert CM.union_variant(A, B, CM.T_DEFAULT, "dup_without_forward").tolist() == [] and CM.union_variant(A, B, CM.T_DEFAULT, "contract").tolist() == [[0, 0, 1]]
    assert CM.union_variant(*_pair_descs(case, 2, 3), CM.T_DEFAULT, "dup_without_forward").tolist() == [[0, 1, 2]]


# ---- M4 ----------------------------------------------------------------------------------------------------------------------------------
def _hypothesis(model, xyuv, idx):
    return NM.hypothesis(xyuv, idx) if model == "homography" else NA.hypothesis(xyuv, idx, model)


@pytest.mark.parametrize("threshold", (3.0, 0.0))
@pytest.mark.parametrize("model", CM.MODELS)
def test_threshold(model, threshold):
    case = CM.built("threshold", model, threshold)
    f = case.facts
    want = CM.contract(model, "threshold", model, threshold)
    CM.assert_rows(case, want)
    CM.assert_winner(case, want, exact_k=False)
    assert want[1]["hypothesis"] == f["first"] and f["count"] == (52 if threshold else 40)
    assert np.abs(NM.centred(case.features[0])).max() <= 20 and np.abs(NM.centred(case.features[1])).max() <= 20
    assert np.bincount(f["kinds"]).tolist() == [40, 12, 12] and len(f["proved"]) >= 4
    xyuv = f["xyuv"].astype(np.float64)
    t2 = np.float64(threshold) * np.float64(threshold)
    for k in f["proved"]:  # every proved hypothesis has exactly the planted inliers; with < the 12 on the threshold are lost
        h, ok = _hypothesis(model, xyuv, CM.sample_of(model, CM.DEFAULT_SEED, 1, k, 64))
        assert ok and np.array_equal(NM.inliers(h, xyuv, t2), f["planted"] != 0)
        lt = CM.inliers_lt(h, xyuv, t2)
        assert np.array_equal(lt, f["kinds"] == 0) if threshold else not lt.any()
        assert not np.array_equal(lt, f["planted"] != 0)


# ---- M5 ----------------------------------------------------------------------------------------------------------------------------------
_COUNTS = {}


def _counts(model):
    """the contract's inlier count of every hypothesis k < 4096 of the M5 pair"""
    if model not in _COUNTS:
        f = CM.built("hypothesis_ties", model, 4096).facts
        xyuv = f["xyuv"].astype(np.float64)
        out = np.zeros(4096, np.int64)
        for k in range(4096):
            h, ok = _hypothesis(model, xyuv, CM.sample_of(model, CM.DEFAULT_SEED, 1, k, len(xyuv)))
            out[k] = int(NM.inliers(h, xyuv, np.float64(9.0)).sum()) if ok else 0
        _COUNTS[model] = out
    return _COUNTS[model]


@pytest.mark.parametrize("iters", CM.TIES_ITERS)
@pytest.mark.parametrize("model", CM.MODELS)
def test_hypothesis_ties(model, iters):
    case = CM.built("hypothesis_ties", model, iters)
    f = case.facts
    want = CM.contract(model, "hypothesis_ties", model, iters)
    CM.assert_rows(case, want)
    CM.assert_winner(case, want, exact_k=True)
    assert f["first_index_is_outlier"] and 0 < f["k_star"] < 44 and f["count"] == 36 and len(f["outliers"]) == 12
    counts = _counts(model)[:iters]
    assert counts.max() == 36 and np.array_equal(np.flatnonzero(counts == 36)[:len(f["clean"])], f["clean"]) and counts[0] < 36
    assert CM.pick(counts) == (f["k_star"], 36)
    loop, tree, largest = CM.pick(counts, loop_ge=True)[0], CM.pick(counts, tree_k=False)[0], CM.pick(counts, largest=True)[0]
    assert largest != f["k_star"]
    assert (f["same_thread"] is not None) == (iters >= 300) and (loop != f["k_star"]) == (iters >= 300)
    # the tree pairs thread t with t + o, which keeps no order among threads: without its k term it goes wrong below 256 too
    assert (f["lower_thread"] is not None) == (iters > CM.PICK_WG) and tree != f["k_star"]
    if iters > CM.PICK_WG:
        assert f["lower_thread"] == CM.PICK_WG and counts[CM.PICK_WG] == 36
    if iters >= 300:
        assert f["same_thread"] == f["k_star"] + CM.PICK_WG


# ---- M6 ----------------------------------------------------------------------------------------------------------------------------------
def test_many_pairs():
    case = CM.built("many_pairs")
    f = case.facts
    want = CM.contract("homography", "many_pairs")
    CM.assert_many(case, want)
    n = CM.MANY_N
    assert len(f["pairs"]) == 237 and 440 <= f["jobs"] <= 474 and f["last_p"] == 118 * 120 + 119 == 14279
    sizes = [len(x["x"]) for x in case.features]
    assert sizes.count(0) >= 2 and sizes.count(1) >= 3 and max(sizes) == 12 and len(sizes) == n
    lone = [p for p, d in f["directions"].items() if d[0] != d[1]]
    none = [p for p, d in f["directions"].items() if not any(d)]
    assert (17, 18) in none and (16, 17) in lone and (18, 19) in lone and len(none) >= 5 and len(lone) >= 8
    ran = [(i, j) for i, j in f["pairs"] if f["counts"][(i, j)] >= CM.MIN_MATCHES]
    assert len(ran) >= 200 and all(want[i * n + j]["hypothesis"] >= 0 for i, j in ran)
    assert len({want[i * n + j]["hypothesis"] for i, j in ran}) >= 3  # k = 0 does not always win: the displaced landmarks
    # the variant: the sampler keyed by the pair's position in the table
    pts = [NM.centred(x) for x in case.features]
    differ = 0
    for pos, (i, j) in enumerate(f["pairs"]):
        e = want[i * n + j]
        if (i, j) in ran and pos != i * n + j:
            xyuv = np.concatenate([pts[i][e["matches"][:, 0]], pts[j][e["matches"][:, 1]]], axis=1)
            k, h, _ = NM.ransac(xyuv, pos, CM.MANY_ITERS, 3.0, CM.DEFAULT_SEED)
            differ += k != e["hypothesis"] or not np.array_equal(h, e["H_sample"])
    assert differ >= 150


# ---- M7 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", CM.SEEDS)
@pytest.mark.parametrize("model", CM.MODELS)
def test_seeds(model, seed):
    case = CM.built("seeds", model, seed)
    want = CM.contract(model, "seeds", model, seed)
    CM.assert_rows(case, want)
    CM.assert_winner(case, want, exact_k=True)
    others = [CM.built("seeds", model, s).facts["first_sample"] for s in CM.SEEDS if s != seed]
    assert case.facts["first_sample"] not in others and case.kw["seed"] == seed
