"""Constructed inputs for the matcher's four kernels (csrc/stx_matches.hip: match_2nn, match_union, match_ransac, match_pick) and the job
and pair tables of csrc/stx_matches_host.cpp.  Every family is built to reach one path of those that random descriptor pools and planted
maps with rounding noise never state they reach, and returns the facts that make it reach it.  Pure numpy, no GPU and no product code:
tests/test_constructed_matches.py asserts the facts against the contracts (tests/numpy_matches.py, tests/numpy_affine.py) and shows that
each family tells the contract from a one-mistake variant of it; tests/test_gpu_constructed_matches.py runs the same inputs on the device.

Every builder returns a Case: the features as the contracts take them (dicts, tests/affine_rigs.features_of's form), the keyword
arguments of the match, and `facts`, a dict stated from the construction, the ratio rule and the contracts' sampler alone — never from a
contract's RANSAC or union output.

Descriptor distances are exact by design.  A descriptor is a set of bits; descriptors that differ from a base in disjoint bit sets
have the sizes of those sets as distances.  Three layouts are used:
  slots      (M1) 6 blocks of 16 bits for the planted train slots, 160 bits of which every filler sets exactly 80
  landmarks  (M3 .. M7) bits 0 .. 39: the 10 bits of the landmark's number, 4 copies each (two landmarks differ in 4 h bits, h >= 1);
             bits 40 .. 127: noise bits, set one by one; bits 128 .. 255: all set in a "dead" descriptor, which is then 128 .. 172 bits
             from every live one: with 1024 * 128 >= 717 * 172 no pair of such distances passes the ratio test at match_conf = 0.3
  one-hot    (M6) 4 bits per landmark number mod 64: every two landmarks an image pair can see are 8 bits apart, so a query without
             its copy ties and stays unmatched

Exact arithmetic (M4, M5, M7): the coordinates are small integers, and `Exact` replays a hypothesis and the inlier test of the
contracts in Python integers, operation by operation in the contracts' order, recording whether every intermediate value is an fp64
number.  Where all are, the fp64 result is the integer result, and what the integers say about a match is what every correct
implementation must say."""
import functools

import numpy as np

from tests import numpy_affine as NA
from tests import numpy_matches as NM

# Constants of the kernels the families are shaped around.  tests/test_constructed_matches.py reads each of them back from the sources:
# a moved constant fails that test instead of letting the families quietly miss their edges.
NN_WG = 256          # STX_MATCH_NN_WG: queries per workgroup of match_2nn and train descriptors per LDS tile
HYP_PER_WG = 4       # STX_MATCH_HYP_PER_WG: hypotheses (wavefronts) per workgroup of match_ransac
NO_D = 0xFFFF        # STX_MATCH_NO_D: "no distance yet"
UNION_CHUNK = 256    # match_union_kernel: queries (and train descriptors) per round of block_place
PICK_WG = 256        # match_pick_kernel: thread tid holds the hypotheses tid, tid + 256, ...
MIN_MATCHES = 6      # both RANSAC kernels: m < 6 runs nothing
MIN_TRAIN = 2        # add_job: a direction with nb < 2 has no job
T_DEFAULT = 717      # ratio_threshold(0.3)
DEFAULT_SEED = 0x5EED
MODELS = ("homography", "affine_partial", "affine_full")
SAMPLE_SIZE = {"homography": 4, "affine_partial": 2, "affine_full": 3}
POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


class Case:
    def __init__(self, features, kw, facts):
        self.features, self.kw, self.facts = list(features), dict(kw), facts
        for f in self.features:
            for v in f.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)


def features_of(desc, xy, size=(640, 480)):
    """the contracts' features dict of descriptors (n, 32) u8 at integer pixels xy (n, 2) of one level"""
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    n = len(xy)
    return {"img_size": size, "level_sizes": [size], "level": np.zeros(n, np.int32), "x": xy[:, 0].copy(), "y": xy[:, 1].copy(),
            "bin": np.zeros(n, np.int32), "R": np.zeros(n, np.int64), "descriptors": np.ascontiguousarray(np.asarray(desc, np.uint8).reshape(n, 32))}


def desc_of(bitsets):
    """(n, 32) u8: descriptor r has exactly the bits of bitsets[r] set"""
    out = np.zeros((len(bitsets), 32), np.uint8)
    for r, s in enumerate(bitsets):
        for b in s:
            out[r, b >> 3] |= 1 << (b & 7)
    return out


def hamming(A, B):
    A, B = np.asarray(A, np.uint8).reshape(-1, 32), np.asarray(B, np.uint8).reshape(-1, 32)
    d = np.zeros((len(A), len(B)), np.int64)
    for k in range(32):
        d += POP[A[:, k, None] ^ B[None, :, k]]
    return d


def _spread(n, salt=0):
    """n distinct integer pixels inside a 640 x 480 image"""
    k = np.arange(n) + salt
    return np.stack([20 + (k * 37) % 600, 20 + (k * 91) % 440], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# M1 tiles (match_2nn)
# ---------------------------------------------------------------------------------------------------------------------------------------
TILE_TRAINS = (257, 512, 513, 600)
TILE_QUERIES = (1, 256, 257)
SLOT_BITS = 16
SLOT_PAIRS = [(a, b) for a in range(6) for b in range(6) if a != b]  # (rank of the nearest slot, rank of the second nearest)


def tile_slots(nb):
    return sorted(s for s in {0, NN_WG - 1, NN_WG, 2 * NN_WG - 1, 2 * NN_WG, nb - 1} if 0 <= s < nb)


def _slot_block(a):
    return list(range(SLOT_BITS * a, SLOT_BITS * a + SLOT_BITS))


def slot_query(a, b):
    """all of block a but its first x = a % 3 bits, and the first 3 bits of block b: x + 3 bits from slot a's descriptor (block a),
    29 - x from slot b's, 35 - x from every other slot's, 19 - x + 80 from a filler"""
    return set(_slot_block(a)[a % 3:]) | set(_slot_block(b)[:3])


def slot_d1(a):
    return a % 3 + 3


def tile_positions(nq):
    """where the 30 planted queries sit in a query image of nq descriptors: (position, a, b); the first query and those either side of
    the workgroup's edge have slot ranks every train image has"""
    if nq == 1:
        return [(0, 1, 2)]  # nearest in slot 255, second nearest in slot 256: the last slot of one tile, the first of the next
    edge = [0, 63, 64, 127, 128, 191, 255, 256] if nq > NN_WG else [0, 63, 64, 127, 128, 191, 192, 255]
    rest = [p for p in range(2, 254, 11) if p not in edge][:len(SLOT_PAIRS) - len(edge)]
    pos = sorted(edge + rest)
    assert len(pos) == len(set(pos)) == len(SLOT_PAIRS) and pos[-1] < nq
    fixed = {p: ab for p, ab in ((0, (1, 0)), (NN_WG - 1, (2, 0)), (NN_WG, (0, 2))) if p in pos}  # matched in every train image: ranks < 3
    rest = [ab for ab in SLOT_PAIRS if ab not in fixed.values()]
    order = np.random.default_rng(nq).permutation(len(rest)).tolist()
    free = iter(rest[k] for k in order)
    return [(p, *(fixed[p] if p in fixed else next(free))) for p in pos]


def tiles():
    """images 0 .. 2: queries (1, 256, 257 descriptors), images 3 .. 6: trains (257, 512, 513, 600).  A train image holds the slot
    descriptors at tile_slots(nb) and fillers elsewhere; a query image holds the planted queries at tile_positions and all-zero
    descriptors elsewhere (16 bits from every slot: a tie).
    facts["rows"][(qi, ti)]: the whole match list of the pair — query (a, b) is matched iff slot rank a exists in the train image, to
    that slot, at distance a % 3 + 3: then d2 is 29 - x or 35 - x; without slot a it is 29 - x against 35 - x or a tie, both unmatched.
    The backward direction adds nothing: every slot descriptor has its 5 queries (a, .) at the same d1, a tie, and every
    filler ties on the all-zero queries; a single query has no backward direction at all"""
    rng = np.random.default_rng(1)
    feats, rows = [], {}
    planted = {nq: tile_positions(nq) for nq in TILE_QUERIES}
    for nq in TILE_QUERIES:
        sets = [set() for _ in range(nq)]
        for p, a, b in planted[nq]:
            sets[p] = slot_query(a, b)
        feats.append(features_of(desc_of(sets), _spread(nq, nq)))
    filler_min = 256
    for nb in TILE_TRAINS:
        slots = tile_slots(nb)
        sets = []
        for t in range(nb):
            if t in slots:
                sets.append(set(_slot_block(slots.index(t))))
            else:
                sets.append(set((96 + rng.permutation(160)[:80]).tolist()))
                filler_min = min(filler_min, len(sets[-1]))
        feats.append(features_of(desc_of(sets), _spread(nb, 7 * nb)))
    # the margins relied on: a filler is farther from every query than any slot; the ratio rule on the three distance pairs
    assert filler_min + (SLOT_BITS - 2 + 3) > 35 and filler_min > SLOT_BITS
    for x in range(3):
        assert NM.ratio_test(x + 3, 29 - x, T_DEFAULT) and NM.ratio_test(x + 3, 35 - x, T_DEFAULT) and not NM.ratio_test(29 - x, 35 - x, T_DEFAULT)
    for qi, nq in enumerate(TILE_QUERIES):
        for tk, nb in enumerate(TILE_TRAINS):
            slots = tile_slots(nb)
            rows[(qi, len(TILE_QUERIES) + tk)] = [(p, slots[a], slot_d1(a)) for p, a, b in planted[nq] if a < len(slots)]
    order_pairs = {(nq, nb): sorted({(tile_slots(nb)[a], tile_slots(nb)[b]) for _, a, b in planted[nq] if max(a, b) < len(tile_slots(nb))})
                   for nq in TILE_QUERIES for nb in TILE_TRAINS}
    return Case(feats, dict(ransac_iters=8), dict(rows=rows, slot_pairs=order_pairs, queries=TILE_QUERIES, trains=TILE_TRAINS))


def _scan(d, idx):
    """i1, d1, d2 of a scan over the columns of d (na, k) in order with strict <: idx[first minimum], the two smallest with multiplicity;
    d2 = NO_D with one column"""
    i = np.argmin(d, axis=1)
    rows = np.arange(len(d))
    d1 = d[rows, i].copy()
    if d.shape[1] < 2:
        return np.asarray(idx)[i].astype(np.int32), d1.astype(np.int32), np.full(len(d), NO_D, np.int32)
    e = d.copy()
    e[rows, i] = 1 << 20
    return np.asarray(idx)[i].astype(np.int32), d1.astype(np.int32), e.min(axis=1).astype(np.int32)


def two_nn_reset(A, B):
    """variant: the running pair (d1, d2) starts over at each tile — what is left is the last tile's"""
    B = np.asarray(B).reshape(-1, 32)
    t0 = NN_WG * ((len(B) - 1) // NN_WG)
    return _scan(hamming(A, B[t0:]), np.arange(t0, len(B)))


def two_nn_stale(A, B):
    """variant: the last, partial tile is compared over all 256 slots — the slots past its end still hold the tile before, and are
    taken for the train descriptors t0 + t"""
    B = np.asarray(B).reshape(-1, 32)
    nb = len(B)
    t0 = NN_WG * ((nb - 1) // NN_WG)
    cnt = nb - t0
    if cnt == NN_WG or t0 == 0:
        return _scan(hamming(A, B), np.arange(nb))
    seq = np.concatenate([B, B[t0 - NN_WG + cnt:t0]])
    return _scan(hamming(A, seq), np.arange(len(seq)))


def forward_rows(A, B, T, two_nn=NM.two_nn):
    """the forward matches (q, i1, d1) of A in B by the ratio rule on the output of `two_nn`"""
    if len(B) < MIN_TRAIN or len(A) == 0:
        return []
    i1, d1, d2 = two_nn(A, B)
    return [(q, int(i1[q]), int(d1[q])) for q in range(len(A)) if NM.ratio_test(d1[q], d2[q], T)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# M2 ratio edges (nn_matched)
# ---------------------------------------------------------------------------------------------------------------------------------------
RATIO_PAIRS = ((0, 1), (7, 10), (70, 100), (71, 101), (1, 1), (5, 5), (0, 0), (1, 2), (255, 256), (256, 256))
RATIO_CONFS = (0.3, 0.0, 1.0)  # T = 717, 1024, 0


def ratio_edges(match_conf):
    """a chain (range_width = 1) of an all-zero query image (1 descriptor) and a train image of two descriptors with d1 and d2 bits set,
    the nearer at index c % 2, per pair c of RATIO_PAIRS.  Pair (2 c, 2 c + 1) has the forward direction only; pair (2 c + 1, 2 c + 2)
    — train image c before the next all-zero query — has the backward direction only and the same two distances.
    facts: T; matched[c] by the ratio rule; rows of every pair"""
    T = NM.ratio_threshold(match_conf)
    feats, matched, rows = [], [], {}
    for c, (d1, d2) in enumerate(RATIO_PAIRS):
        near, far = set(range(d1)), set(range(256 - d2, 256))
        feats.append(features_of(desc_of([set()]), [[100 + c, 50]]))
        feats.append(features_of(desc_of([near, far] if c % 2 == 0 else [far, near]), [[110 + c, 60], [120 + c, 70]]))
        ok = 1024 * d1 < T * d2
        matched.append(ok)
        rows[(2 * c, 2 * c + 1)] = [(0, c % 2, d1)] if ok else []
        if c + 1 < len(RATIO_PAIRS):
            rows[(2 * c + 1, 2 * c + 2)] = [(c % 2, 0, d1)] if ok else []
    return Case(feats, dict(match_conf=match_conf, range_width=1, ransac_iters=4), dict(T=T, matched=matched, rows=rows, pairs=RATIO_PAIRS))


def ratio_float(d1, d2, match_conf):
    """variant: the test in floating point"""
    return float(d1) < (1.0 - match_conf) * float(d2)


def ratio_le(d1, d2, T):
    """variant: <= in place of <"""
    return 1024 * int(d1) <= int(T) * int(d2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# M3 placements (match_union)
# ---------------------------------------------------------------------------------------------------------------------------------------
CODE_COPIES = 4
NOISE0 = 40
TAG0 = 128


def code(k):
    return {CODE_COPIES * b + c for b in range(10) if k >> b & 1 for c in range(CODE_COPIES)}


def live(k, noise=()):
    return code(k) | {NOISE0 + n for n in noise}


def dead(k):
    return code(k) | set(range(TAG0, 256))


def _assert_dead_margin(dead_desc, other_desc, T=T_DEFAULT):
    """no two distances between a dead descriptor and the other image's pass the ratio test"""
    if len(dead_desc) and len(other_desc):
        d = hamming(dead_desc, other_desc)
        assert 1024 * int(d.min()) >= T * int(d.max()), (int(d.min()), int(d.max()))


PLACEMENTS = ("seven", "hole", "all", "none")
SEVEN = (63, 64, 255, 256, 511, 512, 599)
NQ = 600


def exact_copy(k):
    """landmark k in the train image: k % 3 noise bits away"""
    return live(k, range(k % 3))


def placements(which):
    """two images, 600 queries in the first.  Landmark q's copy in the train image is q % 3 bits away and every other live descriptor
    at least 4: matched both ways, the backward match a duplicate.
      seven  only the queries SEVEN are live, the rest dead: 7 rows, one each side of the wavefront and chunk edges
      hole   the chunk 256 .. 511 is dead: 344 rows, a chunk without a match between two busy ones
      all    600 rows, and for 20 landmarks (k % 3 == 0) two more copies A, B at 2 bits each in the train image at t >= 256: the
             forward match stays the exact copy (0 against 2), A and B are backward extras (2 against >= 6)
      none   the train image holds no copy: its first 256 descriptors are dead, the rest are dead ones mixed with pairs A, B (2 bits
             each: a forward tie) of 100 landmarks and pairs X (3 bits), Y (4 bits) of 12 landmarks.  3 against 4 fails the ratio
             test forward, so no query is matched (a query without a pair sees some landmark's pair at 4 h + 2 twice, or X and Y at
             4 h + 3 and 4 h + 4), and the backward pass starts at base 0.  All of A, B, X, Y are backward matches (2, 3, 4 against
             at least 6, 7, 8) and all are kept — X although its query's nearest neighbour is X itself: that forward match failed
    facts: rows (the whole match list), forward (how many of them are forward), extras_by_chunk, kept_same_t (the X rows)"""
    rng = np.random.default_rng(len(which))
    xy_i = _spread(NQ)
    shift = np.array([5, -3])
    if which in ("seven", "hole"):
        alive = set(SEVEN) if which == "seven" else set(range(NQ)) - set(range(UNION_CHUNK, 2 * UNION_CHUNK))
        qi = [live(q) if q in alive else dead(q) for q in range(NQ)]
        order = rng.permutation(sorted(alive)).tolist()
        tj = [exact_copy(k) for k in order]
        xy_j = xy_i[order] + shift
        where = {k: t for t, k in enumerate(order)}
        rows = [(q, where[q], q % 3) for q in sorted(alive)]
        facts = dict(rows={(0, 1): rows}, forward=len(rows), extras_by_chunk={}, kept_same_t=[])
        A, B = desc_of(qi), desc_of(tj)
        _assert_dead_margin(A[[q for q in range(NQ) if q not in alive]], B)
    elif which == "all":
        extra = [k for k in range(0, NQ, 3)][5::10][:20]
        first = rng.permutation(NQ).tolist()
        head, tail = first[:UNION_CHUNK], [("E", k) for k in first[UNION_CHUNK:]] + [(c, k) for k in extra for c in "AB"]
        tail = [tail[t] for t in rng.permutation(len(tail)).tolist()]
        items = [("E", k) for k in head] + tail
        noise = {"A": (10, 11), "B": (12, 13)}
        tj = [exact_copy(k) if c == "E" else live(k, noise[c]) for c, k in items]
        xy_j = xy_i[[k for _, k in items]] + shift
        where = {k: t for t, (c, k) in enumerate(items) if c == "E"}
        rows = [(q, where[q], q % 3) for q in range(NQ)]
        back = [(k, t, 2) for t, (c, k) in enumerate(items) if c != "E"]
        facts = dict(rows={(0, 1): rows + back}, forward=NQ, kept_same_t=[],
                     extras_by_chunk={c: sum(1 for _, t, _ in back if t // UNION_CHUNK == c) for c in range(-(-len(items) // UNION_CHUNK))})
        qi = [live(q) for q in range(NQ)]
        A, B = desc_of(qi), desc_of(tj)
        assert facts["extras_by_chunk"][0] == 0 and facts["extras_by_chunk"][1] > 0 and facts["extras_by_chunk"][2] > 0
    else:
        pairs_ab, pairs_xy = list(range(3, 303, 3)), list(range(310, 346, 3))
        live_items = [(c, k) for k in pairs_ab for c in "AB"] + [(c, k) for k in pairs_xy for c in "XY"]
        tail = live_items + [("D", 600 + z) for z in range(700 - UNION_CHUNK - len(live_items))]
        tail = [tail[t] for t in rng.permutation(len(tail)).tolist()]
        items = [("D", z) for z in range(UNION_CHUNK)] + tail
        noise = {"A": (10, 11), "B": (12, 13), "X": (20, 21, 22), "Y": (23, 24, 25, 26)}
        tj = [dead(k) if c == "D" else live(k, noise[c]) for c, k in items]
        xy_j = np.array([xy_i[k] + shift if c != "D" else (30 + k % 500, 30 + k % 300) for c, k in items])
        back = [(k, t, len(noise[c])) for t, (c, k) in enumerate(items) if c != "D"]
        facts = dict(rows={(0, 1): back}, forward=0, kept_same_t=[(k, t, 3) for t, (c, k) in enumerate(items) if c == "X"],
                     extras_by_chunk={c: sum(1 for _, t, _ in back if t // UNION_CHUNK == c) for c in range(-(-len(items) // UNION_CHUNK))})
        qi = [live(q) for q in range(NQ)]
        A, B = desc_of(qi), desc_of(tj)
        _assert_dead_margin(B[[t for t, (c, _) in enumerate(items) if c == "D"]], A)
        assert facts["extras_by_chunk"][0] == 0 and facts["extras_by_chunk"][1] > 0 and facts["extras_by_chunk"][2] > 0
        assert len(facts["kept_same_t"]) == len(pairs_xy) and not NM.ratio_test(3, 4, T_DEFAULT) and NM.ratio_test(3, 7, T_DEFAULT)
    assert NM.ratio_test(2, 4, T_DEFAULT) and NM.ratio_test(2, 6, T_DEFAULT) and NM.ratio_test(4, 8, T_DEFAULT)
    return Case([features_of(A, xy_i), features_of(B, xy_j)], dict(ransac_iters=8), facts)


def pair_shapes():
    """a chain (range_width = 1) of four images: (0, 1) has the backward direction only (3 descriptors before 1), (1, 2) has neither
    (1 and 1) and lies between two busy pairs, (2, 3) has the forward direction only (1 before 3).
    facts["rows"]: (0, 1): landmark 5's copy at 1 bit, landmark 9 at 9 bits: one backward match.  (2, 3): landmark 7's copy at 2 bits
    at index 1, landmark 11 at 8: one forward match"""
    feats = [features_of(desc_of([live(5), live(9), dead(3)]), [[40, 40], [90, 70], [150, 20]]),
             features_of(desc_of([live(5, (0,))]), [[45, 37]]),
             features_of(desc_of([live(7)]), [[200, 100]]),
             features_of(desc_of([live(9, (0, 1, 2)), live(7, (0, 1)), live(11)]), [[10, 10], [205, 97], [300, 300]])]
    d = hamming(feats[1]["descriptors"], feats[0]["descriptors"])[0]
    assert d[0] == 1 and d[1] == 9 and d[2] > 100
    d = hamming(feats[2]["descriptors"], feats[3]["descriptors"])[0]
    assert d.tolist() == [15, 2, 8]
    rows = {(0, 1): [(0, 0, 1)], (1, 2): [], (2, 3): [(0, 1, 2)]}
    return Case(feats, dict(range_width=1, ransac_iters=4), dict(rows=rows, directions={(0, 1): (False, True), (1, 2): (False, False), (2, 3): (True, False)}))


def union_variant(A, B, T, kind):
    """numpy_matches.union with one mistake:
      "dup_without_ratio"    the duplicate test without nn_matched(f, T)
      "dup_without_forward"  the duplicate test applied where the forward direction has no job (its table read as if it had one:
                             the second distance of a single train descriptor is NO_D)
      "before_le"            block_place counts a wavefront's `before` with w <= wave"""
    A, B = np.asarray(A, np.uint8).reshape(-1, 32), np.asarray(B, np.uint8).reshape(-1, 32)
    fm, fi, fd = NM.one_way(A, B, T)
    bm, bi, bd = NM.one_way(B, A, T)
    if kind == "dup_without_forward" and len(B) == 1 and len(A) > 0:
        fi, fd, d2 = NM.two_nn(A, B)
        dup = 1024 * fd.astype(np.int64) < T * d2.astype(np.int64)
    else:
        dup = np.ones(len(A), bool) if kind == "dup_without_ratio" and len(B) >= MIN_TRAIN else fm
    fwd = [(q, int(fi[q]), int(fd[q])) if fm[q] else None for q in range(len(A))]
    bwd = []
    for t in range(len(B)):
        q = int(bi[t])
        bwd.append((q, t, int(bd[t])) if bm[t] and not (dup[q] and fi[q] == t) else None)
    if kind != "before_le":
        return np.array([r for r in fwd + bwd if r is not None], np.int32).reshape(-1, 3)
    out = np.zeros((len(A) + len(B) + 4 * 64, 3), np.int32)  # room for the misplaced rows: this is numpy, not the device's arena
    base = 0
    for rows in (fwd, bwd):
        for c0 in range(0, len(rows), UNION_CHUNK):
            chunk = rows[c0:c0 + UNION_CHUNK]
            per_wave = [sum(r is not None for r in chunk[w * 64:w * 64 + 64]) for w in range(4)]
            for k, r in enumerate(chunk):
                if r is not None:
                    w = k // 64
                    out[base + sum(per_wave[:w + 1]) + sum(x is not None for x in chunk[w * 64:k])] = r
            base += sum(per_wave)
    return out[:base]


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------
class Exact:
    """collects integer intermediates: ok while every one is an fp64 number, peak the largest magnitude"""

    def __init__(self):
        self.ok, self.peak = True, 0

    def __call__(self, v):
        if float(v) != v:
            self.ok = False
        self.peak = max(self.peak, abs(v))
        return v


def _adj_i(m, ex):
    def minor(a, b, c, d):
        return ex(ex(a * b) - ex(c * d))
    return [[minor(m[1][1], m[2][2], m[1][2], m[2][1]), minor(m[0][2], m[2][1], m[0][1], m[2][2]), minor(m[0][1], m[1][2], m[0][2], m[1][1])],
            [minor(m[1][2], m[2][0], m[1][0], m[2][2]), minor(m[0][0], m[2][2], m[0][2], m[2][0]), minor(m[0][2], m[1][0], m[0][0], m[1][2])],
            [minor(m[1][0], m[2][1], m[1][1], m[2][0]), minor(m[0][1], m[2][0], m[0][0], m[2][1]), minor(m[0][0], m[1][1], m[0][1], m[1][0])]]


def _sum3(a, b, c, ex):
    return ex(ex(a + b) + c)


def _basis_i(pts, ex):
    m = [[pts[0][0], pts[1][0], pts[2][0]], [pts[0][1], pts[1][1], pts[2][1]], [1, 1, 1]]
    a = _adj_i(m, ex)
    lam = [_sum3(ex(a[r][0] * pts[3][0]), ex(a[r][1] * pts[3][1]), a[r][2], ex) for r in range(3)]
    return [[ex(m[r][c] * lam[c]) for c in range(3)] for r in range(3)]


def hypothesis_int(model, xyuv, idx, ex):
    """the contracts' hypothesis (numpy_matches.hypothesis, numpy_affine.hypothesis) of integer coordinates in Python integers, every
    product, sum and difference in their order passed through `ex` -> H (9 ints, the sign rule applied), whether it can have inliers"""
    src, dst = [tuple(int(v) for v in xyuv[i][0:2]) for i in idx], [tuple(int(v) for v in xyuv[i][2:4]) for i in idx]
    if model == "homography":
        a, b = _adj_i(_basis_i(src, ex), ex), _basis_i(dst, ex)
        h = [_sum3(ex(b[r][0] * a[0][c]), ex(b[r][1] * a[1][c]), ex(b[r][2] * a[2][c]), ex) for r in range(3) for c in range(3)]
        w0 = _sum3(ex(h[6] * src[0][0]), ex(h[7] * src[0][1]), h[8], ex)
        return ([-v for v in h] if w0 < 0 else h), w0 != 0
    if model == "affine_partial":
        (x0, y0), (x1, y1), (u0, v0), (u1, v1) = src[0], src[1], dst[0], dst[1]
        dx, dy, du, dv = x1 - x0, y1 - y0, u1 - u0, v1 - v0
        W = ex(ex(dx * dx) + ex(dy * dy))
        A = ex(ex(du * dx) + ex(dv * dy))
        B = ex(ex(dv * dx) - ex(du * dy))
        C = ex(ex(u0 * W) - ex(ex(A * x0) - ex(B * y0)))
        D = ex(ex(v0 * W) - ex(ex(B * x0) + ex(A * y0)))
        h = [A, -B, C, B, A, D, 0, 0, W]
    else:
        a = _adj_i([[src[0][0], src[1][0], src[2][0]], [src[0][1], src[1][1], src[2][1]], [1, 1, 1]], ex)
        N = [[dst[0][0], dst[1][0], dst[2][0]], [dst[0][1], dst[1][1], dst[2][1]]]
        h = [_sum3(ex(N[r][0] * a[0][c]), ex(N[r][1] * a[1][c]), ex(N[r][2] * a[2][c]), ex) for r in range(2) for c in range(3)]
        h += [0, 0, _sum3(ex(src[0][0] * a[0][0]), ex(src[1][0] * a[1][0]), ex(src[2][0] * a[2][0]), ex)]
    w = h[8]
    if w < 0:
        h = [-v for v in h[:6]] + [0, 0, -w]
    return h, w != 0


def residual_int(h, row, ex):
    """(ex, ey, W) of numpy_matches.inliers for one match in Python integers"""
    x, y, u, v = (int(c) for c in row)
    X = _sum3(ex(h[0] * x), ex(h[1] * y), h[2], ex)
    Y = _sum3(ex(h[3] * x), ex(h[4] * y), h[5], ex)
    W = _sum3(ex(h[6] * x), ex(h[7] * y), h[8], ex)
    return ex(X - ex(u * W)), ex(Y - ex(v * W)), W


def model_points(f, model):
    """the integer coordinates the model works on: centred for the homography, raw level-0 pixels for the affine models"""
    p = NM.centred(f) if model == "homography" else NA.uncentred(f)
    assert np.array_equal(p, np.rint(p))
    return p.astype(np.int64)


def sample_of(model, seed, p, k, m):
    return NM.sample(seed, p, k, m)[:SAMPLE_SIZE[model]]


def translation_sample(model, xyuv, idx, shift, squares):
    """replays hypothesis k's sample `idx` (all matches of it exact under the translation `shift`) in integers.  -> (proved, scale):
    proved: every value of the hypothesis and of the residuals of all matches is an fp64 number — with squares=True also W W, which makes
    ex ex + ey ey <= 9 (W W) the comparison of the same real numbers on both sides for a match displaced by 3 along an axis — and the
    hypothesis is scale x the translation with scale > 0.  Far matches need no exact squares: rounding is monotonic"""
    ex = Exact()
    h, ok = hypothesis_int(model, xyuv, idx, ex)
    s = h[8]
    if not ok or h != [s, 0, s * shift[0], 0, s, s * shift[1], 0, 0, s]:
        assert not ok, (model, idx, h)  # the algebra: an all-exact sample gives scale x the translation, or is degenerate
        return False, 0
    for row in xyuv:
        ex_, ey_, W = residual_int(h, row, ex)
        assert W == s and ex_ == s * (int(row[0]) + shift[0] - int(row[2])) and ey_ == s * (int(row[1]) + shift[1] - int(row[3]))
    if squares:
        ex(s * s)
    return ex.ok and s > 0, s


# ---------------------------------------------------------------------------------------------------------------------------------------
# M4 threshold (match_inlier)
# ---------------------------------------------------------------------------------------------------------------------------------------
THRESHOLD_SIZE = (64, 48)  # even sides: centred coordinates of integer pixels are integers
THRESHOLD_SHIFT = (4, -3)
THRESHOLD_ITERS = 64
ON_EDGE = [(3, 0), (-3, 0), (0, 3), (0, -3)] * 3                                                   # squared distance 9 = t^2
JUST_OUT = [(3, 1), (-3, 1), (3, -1), (-1, -3), (1, 3), (-1, 3), (2, -3), (-2, 3), (3, 2), (-3, -2), (2, 3), (-3, 2)]  # 10 or 13


def threshold(model, ransac_threshold=3.0, seed=DEFAULT_SEED):
    """64 matches of an integer translation on a 64 x 48 image, every centred coordinate within +-20: 40 exact, 12 displaced by exactly
    3 along an axis, 12 to the squared distance 10 or 13, shuffled.  Match e is query e (every descriptor has its exact copy).
    facts: kinds per match; planted (the 52 within 3; at ransac_threshold = 0 the 40 exact); proved: the hypotheses k < 64 whose sample
    is all exact by the sampler and whose arithmetic `translation_sample` proves exact — each has exactly the planted inliers; first:
    the smallest of them, so the winner's k is at most that; count: 52 (40)"""
    rng = np.random.default_rng(4)
    m = 64
    grid = [(x, y) for x in range(-12, 13) for y in range(-12, 13)]
    src = np.array([grid[k] for k in rng.permutation(len(grid))[:m].tolist()])
    kinds = np.array([0] * 40 + [1] * 12 + [2] * 12)[rng.permutation(m)]
    disp = np.zeros((m, 2), np.int64)
    disp[kinds == 1], disp[kinds == 2] = ON_EDGE, JUST_OUT
    assert sorted(set((disp[kinds == 2] ** 2).sum(axis=1).tolist())) == [10, 13] and ((disp[kinds == 1] ** 2).sum(axis=1) == 9).all()
    dst = src + THRESHOLD_SHIFT + disp
    assert np.abs(src).max() <= 20 and np.abs(dst).max() <= 20
    centre = np.array(THRESHOLD_SIZE) // 2
    order = rng.permutation(m)
    D = desc_of([live(k) for k in range(m)])
    feats = [features_of(D, src + centre, THRESHOLD_SIZE), features_of(D[order], (dst + centre)[order], THRESHOLD_SIZE)]
    where = np.argsort(order)
    xyuv = np.concatenate([model_points(feats[0], model), model_points(feats[1], model)[where]], axis=1)
    assert np.array_equal(xyuv[:, 2:4] - xyuv[:, 0:2], THRESHOLD_SHIFT + disp)
    proved = []
    for k in range(THRESHOLD_ITERS):
        idx = sample_of(model, seed, 1, k, m)
        if all(kinds[i] == 0 for i in idx) and translation_sample(model, xyuv, idx, THRESHOLD_SHIFT, ransac_threshold != 0.0)[0]:
            proved.append(k)
    planted = (kinds <= 1 if ransac_threshold != 0.0 else kinds == 0).astype(np.uint8)
    assert proved, model
    facts = dict(kinds=kinds, planted=planted, proved=proved, first=proved[0], count=int(planted.sum()), rows={(0, 1): [(q, int(where[q]), 0) for q in range(m)]},
                 xyuv=xyuv)
    return Case(feats, dict(ransac_iters=THRESHOLD_ITERS, ransac_threshold=ransac_threshold, seed=seed), facts)


def inliers_lt(h, xyuv, t2):
    """variant of numpy_matches.inliers: < in place of <="""
    x, y, u, v = xyuv[:, 0], xyuv[:, 1], xyuv[:, 2], xyuv[:, 3]
    with np.errstate(all="ignore"):
        X = (h[0] * x + h[1] * y) + h[2]
        Y = (h[3] * x + h[4] * y) + h[5]
        W = (h[6] * x + h[7] * y) + h[8]
        ex, ey = X - u * W, Y - v * W
        return (W > 0) & (ex * ex + ey * ey < t2 * (W * W))


# ---------------------------------------------------------------------------------------------------------------------------------------
# M5 hypothesis ties (match_pick), M7 seeds
# ---------------------------------------------------------------------------------------------------------------------------------------
TIES_SIZE = (128, 96)
TIES_SHIFT = (4, -3)
TIES_ITERS = (255, 256, 257, 300, 4096)
TIES_M, TIES_OUT = 48, 12


def _ties_points():
    rng = np.random.default_rng(5)
    grid = [(x, y) for x in range(-14, 15) for y in range(-14, 15)]
    src = np.array([grid[k] for k in rng.permutation(len(grid))[:TIES_M].tolist()])
    far = np.stack([rng.integers(22, 30, TIES_M) * rng.choice([-1, 1], TIES_M), rng.integers(18, 26, TIES_M) * rng.choice([-1, 1], TIES_M)], axis=1)
    return src, far, rng.permutation(TIES_M)


def _ties_case(model, outliers, iters, seed):
    src, far, order = _ties_points()
    bad = np.zeros(TIES_M, bool)
    bad[list(outliers)] = True
    dst = src + TIES_SHIFT + far * bad[:, None]
    centre = np.array(TIES_SIZE) // 2
    D = desc_of([live(k) for k in range(TIES_M)])
    feats = [features_of(D, src + centre, TIES_SIZE), features_of(D[order], (dst + centre)[order], TIES_SIZE)]
    where = np.argsort(order)
    xyuv = np.concatenate([model_points(feats[0], model), model_points(feats[1], model)[where]], axis=1)
    assert ((far ** 2).sum(axis=1) >= 100).all()  # far: 100 W W against 9 W W is decided whatever the rounding
    return feats, xyuv, bad, where


def clean_ks(model, xyuv, bad, iters, seed, prove=True):
    """the hypotheses k < iters whose sample holds no outlier and is proved to give scale x the translation in exact arithmetic, scale > 0:
    every exact match is then an inlier (its residual is exactly 0) and every far one is not, the count is 36"""
    out = []
    for k in range(iters):
        idx = sample_of(model, seed, 1, k, len(xyuv))
        if not any(bad[i] for i in idx) and (not prove or translation_sample(model, xyuv, idx, TIES_SHIFT, False)[0]):
            out.append(k)
    return out


_TIES_OUTLIERS = {}


def ties_outliers(seed=DEFAULT_SEED):
    """12 of the 48 match indices: the first index of sample(seed, 1, 0, 48) (so k = 0 loses in every model) and 11 drawn by the first
    generator seed 0, 1, ... for which, in all three models, k = 256 is clean and so is k* + 256 < 300 (k* the first clean k)"""
    if seed not in _TIES_OUTLIERS:
        first = NM.sample(seed, 1, 0, TIES_M)[0]
        for trial in range(400):
            rng = np.random.default_rng(trial)
            rest = [i for i in rng.permutation(TIES_M).tolist() if i != first][:TIES_OUT - 1]
            out = sorted([first] + rest)
            good = True
            for prove in (False, True):  # by the sampler alone first, which is quick; then with the arithmetic proved exact
                for model in MODELS:
                    if good:
                        _, xyuv, bad, _ = _ties_case(model, out, 300, seed)
                        ks = clean_ks(model, xyuv, bad, 300, seed, prove)
                        good = bool(ks) and ks[0] > 0 and 256 in ks and ks[0] + PICK_WG in ks
            if good:
                _TIES_OUTLIERS[seed] = (out, trial)
                break
        assert seed in _TIES_OUTLIERS
    return _TIES_OUTLIERS[seed]


def hypothesis_ties(model, iters, seed=DEFAULT_SEED):
    """48 matches of an integer translation, 12 of them far outliers at ties_outliers().  Match e is query e.
    facts, from the sampler and exact arithmetic only: clean (the clean k < iters); k_star = clean[0] > 0; count 36; same_thread: the
    first clean k > k* congruent to k* mod 256 (thread k* mod 256 of match_pick holds both), present from iters = k* + 257 on;
    lower_thread: the first clean k > k* with k mod 256 < k* mod 256 (the tree meets a tie whose lower thread holds the larger k),
    present above 256"""
    out, trial = ties_outliers(seed)
    feats, xyuv, bad, where = _ties_case(model, out, iters, seed)
    clean = clean_ks(model, xyuv, bad, iters, seed)
    ks = clean[0]
    same = next((k for k in clean if k > ks and k % PICK_WG == ks % PICK_WG), None)
    lower = next((k for k in clean if k > ks and k % PICK_WG < ks % PICK_WG), None)
    assert ks > 0 and (same is not None) == (iters >= ks + PICK_WG + 1) and (lower is not None) == (iters > PICK_WG)
    facts = dict(clean=clean, k_star=ks, count=TIES_M - TIES_OUT, first_index_is_outlier=bool(bad[sample_of(model, seed, 1, 0, TIES_M)[0]]), same_thread=same, lower_thread=lower, outliers=out, trial=trial,
                 planted=(~bad).astype(np.uint8), rows={(0, 1): [(q, int(where[q]), 0) for q in range(TIES_M)]}, xyuv=xyuv)
    return Case(feats, dict(ransac_iters=iters, seed=seed), facts)


INT_MAX = 2 ** 31 - 1


def pick(counts, loop_ge=False, tree_k=True, largest=False):
    """match_pick_kernel's arg-max in numpy: thread tid scans k = tid, tid + 256, ... with strict >, a halving tree over 256 threads takes
    the larger count and the smaller k among equals.  Variants: loop_ge (>= in the loop), tree_k=False (the tree without its k term),
    largest (the largest k among equals: >= in the loop, > on k in the tree)"""
    n_, k_ = [-1] * PICK_WG, [INT_MAX] * PICK_WG
    for tid in range(PICK_WG):
        for k in range(tid, len(counts), PICK_WG):
            c = int(counts[k])
            if c > n_[tid] or ((loop_ge or largest) and c == n_[tid]):
                n_[tid], k_[tid] = c, k
    o = PICK_WG // 2
    while o:
        for tid in range(o):
            n, k = n_[tid + o], k_[tid + o]
            tie = n == n_[tid] and tree_k and (k > k_[tid] if largest else k < k_[tid])
            if n > n_[tid] or tie:
                n_[tid], k_[tid] = n, k
        o //= 2
    return k_[0], n_[0]


SEEDS = (0, 0x80000000, 0xFFFFFFFF)
SEED_ITERS = 64


def seeds(model, seed):
    """the M5 pair under `seed` with 64 hypotheses and the outliers at the match indices 0, 4, 8, ..., 44.
    facts: k_star, the first clean k by the sampler under this seed, count 36"""
    out = list(range(0, TIES_M, 4))
    feats, xyuv, bad, where = _ties_case(model, out, SEED_ITERS, seed)
    clean = clean_ks(model, xyuv, bad, SEED_ITERS, seed)
    assert clean
    facts = dict(clean=clean, k_star=clean[0], count=TIES_M - TIES_OUT, planted=(~bad).astype(np.uint8), xyuv=xyuv,
                 rows={(0, 1): [(q, int(where[q]), 0) for q in range(TIES_M)]}, first_sample=sample_of(model, seed, 1, 0, TIES_M))
    return Case(feats, dict(ransac_iters=SEED_ITERS, seed=seed), facts)


# ---------------------------------------------------------------------------------------------------------------------------------------
# M6 many pairs (the job and pair tables)
# ---------------------------------------------------------------------------------------------------------------------------------------
MANY_N, MANY_WIDTH, MANY_ITERS, MANY_STEP = 120, 2, 7, 3


def many_counts():
    """features per image: 12 mostly, a few of 0 .. 11 — 0 and 1 among them, next to each other and alone"""
    c = [12] * MANY_N
    for at, v in ((5, 0), (17, 1), (18, 1), (30, 2), (55, 5), (56, 7), (84, 0), (99, 11), (110, 6), (118, 1), (119, 9)):
        c[at] = v
    return c


def one_hot(g):
    return set(range(4 * (g % 64), 4 * (g % 64) + 4))


def many_pairs():
    """120 images in a chain, range_width = 2.  Image t sees the landmarks 3 t .. 3 t + n_t - 1 (one-hot descriptors: equal ones at
    0 bits, different ones at 8), each at its own place less t x (3, 1): neighbours share up to 9 landmarks, next neighbours up to 6,
    through an integer translation; one landmark in four is displaced in odd images.  ransac_iters = 7: two workgroups of hypotheses per
    pair, the second with three live wavefronts.
    facts: pairs (in table order), directions[(i, j)] = (forward has a job, backward has a job), jobs, counts[(i, j)] = the shared
    landmarks where a direction has a job (a query without its copy ties at 8 bits), last_p"""
    n = many_counts()
    feats = []
    for t, nt in enumerate(n):
        g = np.arange(3 * t, 3 * t + nt)
        xy = np.stack([50 + (g * 29) % 380 + 3 * (MANY_N - t), 40 + (g * 53) % 250 + (MANY_N - t)], axis=1).reshape(-1, 2)
        off = ((g + t) % 4 == 0) & (t % 2 == 1)
        xy = xy + np.where(off[:, None], (9, -7), (0, 0))
        feats.append(features_of(desc_of([one_hot(int(v)) for v in g]), xy, (800, 440)))
    pairs = [(i, j) for i in range(MANY_N) for j in range(i + 1, MANY_N) if j - i <= MANY_WIDTH]
    directions = {(i, j): (n[i] >= 1 and n[j] >= MIN_TRAIN, n[j] >= 1 and n[i] >= MIN_TRAIN) for i, j in pairs}
    counts = {}
    for i, j in pairs:
        shared = max(0, min(3 * i + n[i], 3 * j + n[j]) - 3 * j)
        counts[(i, j)] = shared if any(directions[(i, j)]) else 0
    assert 3 * MANY_WIDTH + 12 <= 64  # the landmarks of an image pair are within 64 of each other: distinct one-hot blocks
    facts = dict(pairs=pairs, directions=directions, jobs=sum(a + b for a, b in directions.values()), counts=counts,
                 last_p=pairs[-1][0] * MANY_N + pairs[-1][1], hb=-(-MANY_ITERS // HYP_PER_WG), last_block_live=MANY_ITERS % HYP_PER_WG)
    return Case(feats, dict(range_width=MANY_WIDTH, ransac_iters=MANY_ITERS), facts)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases built once, the contracts' results of them computed once, and the facts asserted on a result (a contract's or the device's)
# ---------------------------------------------------------------------------------------------------------------------------------------
BUILDERS = {"tiles": tiles, "ratio_edges": ratio_edges, "placements": placements, "pair_shapes": pair_shapes, "threshold": threshold,
            "hypothesis_ties": hypothesis_ties, "seeds": seeds, "many_pairs": many_pairs}


@functools.lru_cache(maxsize=None)
def built(name, *args):
    return BUILDERS[name](*args)


@functools.lru_cache(maxsize=None)
def contract(model, name, *args):
    """the contract's n * n entries of a case under `model`: computed once, never written to"""
    c = built(name, *args)
    return NM.match(c.features, **c.kw) if model == "homography" else NA.match(c.features, model=model, **c.kw)


def field(e, name):
    return e[name] if isinstance(e, dict) else getattr(e, name)


def assert_rows(case, result):
    """the match lists the facts name are exactly the facts' rows"""
    n = len(case.features)
    for (i, j), rows in case.facts["rows"].items():
        got = field(result[i * n + j], "matches")
        assert (field(result[i * n + j], "src_img_idx"), field(result[i * n + j], "dst_img_idx")) == (i, j)
        assert got.tolist() == [list(r) for r in rows], (i, j, len(got), len(rows))


def assert_winner(case, result, exact_k):
    """M4, M5, M7 on entry (0, 1): the winner's count, its mask where the winner is a proved hypothesis, and its k — exactly
    facts["k_star"] (exact_k) or at most facts["first"]"""
    f, e = case.facts, result[1]
    assert field(e, "num_inliers") == f["count"], (field(e, "num_inliers"), f["count"])
    k = field(e, "hypothesis")
    if exact_k:
        assert k == f["k_star"], (k, f["k_star"])
    else:
        assert 0 <= k <= f["first"], (k, f["first"])
    if exact_k or k in f["proved"]:
        assert np.array_equal(field(e, "inliers_mask"), f["planted"])


def assert_many(case, result):
    f, n = case.facts, len(case.features)
    done = [(field(e, "src_img_idx"), field(e, "dst_img_idx")) for e in result if 0 <= field(e, "src_img_idx") < field(e, "dst_img_idx")]
    assert done == f["pairs"] and len(done) == 237
    for (i, j), c in f["counts"].items():
        assert len(field(result[i * n + j], "matches")) == c, (i, j)
    for i in range(n):
        for j in range(i + MANY_WIDTH + 1, n):
            assert field(result[i * n + j], "src_img_idx") == -1 and len(field(result[i * n + j], "matches")) == 0
