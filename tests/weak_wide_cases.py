"""Named, seeded inputs of the wide OICR targets kernel (unit_oicr_targets_wide: 1024 threads, thread t owns rows t, t + 1024, ..., at most 8),
for test_weak_wide_cpu.py / test_weak_wide_ops_gpu.py. References: weak_loss_ref.py (float64) and oracle/unit_oracle.py, both row-generic.

Built with the pieces and under the conditions of weak_loss_cases.py (integer boxes: every IoU one correctly rounded division; junk columns
around the live ones; empty slots hold SENTINEL in mode 0 -- larger than every live value -- and NaN in mode 1; no IoU within GAP of a
threshold unless placed on it by hand; in mode 1 every chosen maximum leads its runner-up by a relative GAP = 1e-4, three orders of magnitude
above the fp32 rounding of a softmax value, asserted when the case is built: no comparison is left out of any test).

What is new here is WHERE the rows sit: a "slot" j of thread t is row t + 1024 j, a wave is 64 consecutive threads. PLACES (below) says, per S, which
rows carry the hand-placed values of a mode 0 case."""
import functools

import torch

import weak_loss_cases as C
import weak_loss_ref as ref

SENTINEL, GAP, NAN = C.SENTINEL, C.GAP, C.NAN
THREADS, SLOTS = 1024, 8
SIZES = [1000, 1024, 1025, 2047, 2048, 2049, 5000, 8192]

# the labelled classes of image 0 of a hand-placed case, visited in this (ascending) order
CLS_SAME_THREAD, CLS_TWO_THREADS, CLS_AFTER_ZEROING, CLS_TWO_WAVES, CLS_LOW_ROW_HIGH_THREAD, CLS_SHARED_A, CLS_SHARED_B = 1, 4, 5, 7, 9, 11, 13
HAND_LABELS = lambda K: [CLS_SAME_THREAD, CLS_TWO_THREADS, CLS_AFTER_ZEROING, CLS_TWO_WAVES, CLS_LOW_ROW_HIGH_THREAD, CLS_SHARED_A, CLS_SHARED_B,
                         K - 1]
GT_E, GT_F, GT_G = (700, 700, 730, 730), (800, 800, 820, 830), (900, 900, 940, 910)


def places(S):
    """-> dict of the rows of image 0 that carry hand-placed values, for a case of S rows (S >= 1000):
      same:    (a, a + 1024), two rows of ONE thread (S >= 1025; below that two rows of two waves)
      threads: two lanes of one wave, in the threads' SECOND slot when S >= 1100: the winner's zeroing is a bit above bit 0 of its mask
      runner:  the row class CLS_AFTER_ZEROING must fall back to once the winner of CLS_TWO_THREADS -- its own largest entry -- is zeroed
      waves:   two rows of two different waves in the highest slot that holds both
      cross:   (lo, hi) with lo < hi, lo owned by a thread of the LAST wave and hi by a thread of wave 0 (its second slot; S >= 1025)
      shared:  one row that is the maximum of two classes, and the row the second of them falls back to
      tb:      offset of the threshold rows (weak_loss_cases.THRESHOLD_ROWS, EQUAL_IOU_ROW): 1024 when S >= 1100
      empty:   [lo, hi) ranges of empty slots: inside a wave, a whole wave, and (S > 1470) a range that crosses waves in the second slot"""
    wide = S > THREADS
    base = THREADS * max(0, (S - 324) // THREADS)
    p = dict(same=(min(5, S - 1025), min(5, S - 1025) + THREADS) if wide else (5, S - 5),
             threads=(THREADS + 20, THREADS + 33) if S >= 1100 else (20, 33), runner=200,
             waves=(base + 130, base + 323), cross=(1000, min(1030, S - 1)) if wide else (S - 100, S - 10),
             shared=(40, 210), tb=THREADS if S >= 1100 else 0,
             empty=[(60, 63), (64, 128)] + ([(1400, 1470)] if S > 1470 else []))
    return p


# name -> (mode, S, K, B, (fg, bg), seed)
CASES = {
    # mode 0, hand-placed (_hand): three images -- the placed one, one without a label, one wholly empty (with labels)
    "m0_s1000_k20": (0, 1000, 20, 3, (0.5, 0.1), 131),          # below the narrow kernel's limit: both kernels run, bit for bit
    "m0_s1024_k80": (0, 1024, 80, 3, (0.6, 0.3), 132),
    "m0_s1025_k95": (0, 1025, 95, 3, (0.5, 0.1), 133),          # one row in the second slot: thread 0 alone owns two
    "m0_s2047_k20": (0, 2047, 20, 3, (0.6, 0.3), 134),
    "m0_s2048_k80": (0, 2048, 80, 3, (0.5, 0.1), 135),          # two full slots
    "m0_s2049_k95": (0, 2049, 95, 3, (0.6, 0.3), 136),
    "m0_s5000_k20": (0, 5000, 20, 3, (0.5, 0.1), 137),          # the largest value a shipped yaml sets
    "m0_s8192_k80": (0, 8192, 80, 3, (0.6, 0.3), 138),          # every slot of every thread
    "m0_s8192_k95": (0, 8192, 95, 3, (0.5, 0.1), 139),
    # mode 0, more labels than live rows (_few): one image, rows 3 and 1030 live, four labels
    "m0_s2049_k20_few": (0, 2049, 20, 1, (0.5, 0.1), 140),
    # mode 1, random logits (softmax in the kernel); images `third`, `ragged` and one with a wave and a cross-wave range empty
    "m1_s1000_k95": (1, 1000, 95, 1, (0.5, 0.1), 141),
    "m1_s1024_k20": (1, 1024, 20, 3, (0.6, 0.3), 142),
    "m1_s1025_k80": (1, 1025, 80, 1, (0.5, 0.1), 143),
    "m1_s2047_k95": (1, 2047, 95, 3, (0.5, 0.1), 144),
    "m1_s2048_k20": (1, 2048, 20, 1, (0.6, 0.3), 145),
    "m1_s2049_k80": (1, 2049, 80, 3, (0.5, 0.1), 146),
    "m1_s5000_k95": (1, 5000, 95, 1, (0.6, 0.3), 147),
    "m1_s5000_k20": (1, 5000, 20, 3, (0.5, 0.1), 148),
    "m1_s8192_k80": (1, 8192, 80, 3, (0.5, 0.1), 149),
    "m1_s8192_k95": (1, 8192, 95, 1, (0.6, 0.3), 150),
}
HAND = [n for n, v in CASES.items() if v[0] == 0 and not n.endswith("_few")]
FEW = "m0_s2049_k20_few"
FEW_ROWS, FEW_LABELS = (3, 1030), [2, 6, 10, 17]


def _frame(S, K, B, ncol, col0, ld, g, fill):
    src = torch.full((B * S, ld), fill)
    rois5 = torch.zeros(B * S, 5)
    rois5[:, 0] = torch.arange(B).repeat_interleave(S).float()
    rois5[:, 1:] = C._int_boxes(g, B * S)
    return src, rois5, torch.zeros(B * S, dtype=torch.int32), torch.zeros(B, K, dtype=torch.uint8)


def _hand(S, K, B, thr, seed):
    """image 0, in the order of its classes (rows from places(S)):
      CLS_SAME_THREAD         0.75 in both `same` rows: the lower one (box GT_A) wins
      CLS_TWO_THREADS         0.5 in both `threads` rows: the lower one (box GT_B) wins and is zeroed
      CLS_AFTER_ZEROING       0.9375 in that zeroed row, 0.625 in `runner` (box GT_E): `runner` must win
      CLS_TWO_WAVES           0.875 in both `waves` rows: the lower one (box GT_C) wins
      CLS_LOW_ROW_HIGH_THREAD 0.8125 in both `cross` rows: the lower row (box GT_F) wins although the higher one sits in wave 0
      CLS_SHARED_A / _B       0.6875 / 0.90625 in shared[0] (box GT_G), 0.4375 for _B in shared[1]: _A takes shared[0], _B falls back to shared[1]
      K - 1                   zero in every live row: the lowest row, row 0 (box GT_D), score 0 -- at S = 1025 row 0 won CLS_SAME_THREAD already
    Image 1 has no label, image 2 only empty slots (and labels)."""
    assert B == 3 and S >= 1000
    g = C._gen(seed)
    col0, ld = 2, K + 5
    src, rois5, valid, multihot = _frame(S, K, B, K, col0, ld, g, SENTINEL)
    src[:, col0:col0 + K] = torch.randint(0, 64, (B * S, K), generator=g).float() / 256.0          # < 0.25, exact
    pl = places(S)
    multihot[0, HAND_LABELS(K)] = 1
    multihot[2, [0, 3]] = 1
    valid[2 * S:] = -1
    for lo, hi in pl["empty"]:
        valid[lo:hi] = -1
    p, b = src[:S, col0:col0 + K], rois5[:S, 1:]
    box = lambda t: torch.tensor(t).float()
    p[:, K - 1] = 0.0
    for rows, c, v in ((pl["same"], CLS_SAME_THREAD, 0.75), (pl["threads"], CLS_TWO_THREADS, 0.5), (pl["waves"], CLS_TWO_WAVES, 0.875),
                       (pl["cross"], CLS_LOW_ROW_HIGH_THREAD, 0.8125)):
        p[rows[0], c], p[rows[1], c] = v, v
    p[pl["threads"][0], CLS_AFTER_ZEROING], p[pl["runner"], CLS_AFTER_ZEROING] = 0.9375, 0.625
    p[pl["shared"][0], CLS_SHARED_A], p[pl["shared"][0], CLS_SHARED_B], p[pl["shared"][1], CLS_SHARED_B] = 0.6875, 0.90625, 0.4375
    far = lambda i: box((1000 + 50 * i, 1000, 1030 + 50 * i, 1040))          # the losers of the ties and the fall-back rows: far from everything
    for i, r in enumerate((pl["same"][1], pl["threads"][1], pl["waves"][1], pl["cross"][1], pl["shared"][1])):
        b[r] = far(i)
    b[pl["same"][0]], b[pl["threads"][0]], b[pl["waves"][0]] = box(C.GT_A), box(C.GT_B), box(C.GT_C)
    b[pl["runner"]], b[pl["cross"][0]], b[pl["shared"][0]] = box(GT_E), box(GT_F), box(GT_G)
    if pl["same"][0] != 0:
        b[0] = box(C.GT_D)
    tb = pl["tb"]
    for r, (bx, _) in C.THRESHOLD_ROWS.items():
        b[r + tb] = box(bx)
    b[C.EQUAL_IOU_ROW + tb] = box((20, 10, 50, 30))
    constructed = {r + tb for r in C.THRESHOLD_ROWS} | {C.EQUAL_IOU_ROW + tb}
    src[valid < 0] = SENTINEL
    out, info = C._settle(g, src, 0, K, rois5, valid, S, B, multihot, thr, col0, constructed)
    return dict(src=src, col0=col0, rois5=rois5, valid=valid, multihot=multihot, constructed=constructed, ref=out, info=info, places=pl)


def _few(S, K, B, thr, seed):
    """one image whose only live rows are FEW_ROWS (two slots of two threads), four labels: the third and the fourth class choose among zeros"""
    assert B == 1
    g = C._gen(seed)
    col0, ld = 2, K + 5
    src, rois5, valid, multihot = _frame(S, K, B, K, col0, ld, g, SENTINEL)
    valid[:] = -1
    multihot[0, FEW_LABELS] = 1
    for i, r in enumerate(FEW_ROWS):
        valid[r] = 0
        src[r, col0:col0 + K] = torch.randint(1, 64, (K,), generator=g).float() / 256.0
    src[FEW_ROWS[1], col0 + FEW_LABELS[0]] = 0.5          # the first class takes the HIGHER row, the second the lower, then zeros: the lower twice
    rois5[FEW_ROWS[0], 1:], rois5[FEW_ROWS[1], 1:] = torch.tensor([10., 10., 30., 30.]), torch.tensor([10., 10., 30., 40.])
    out, info = C._settle(g, src, 0, K, rois5, valid, S, B, multihot, thr, col0, set(FEW_ROWS))
    return dict(src=src, col0=col0, rois5=rois5, valid=valid, multihot=multihot, constructed=set(FEW_ROWS), ref=out, info=info, places=None)


def _random(S, K, B, thr, seed):
    g = C._gen(seed)
    col0, ld = 3, K + 1 + 7
    src, rois5, valid, multihot = _frame(S, K, B, K + 1, col0, ld, g, 50.0)          # a junk logit of 50 would own the softmax
    src[:, col0:col0 + K + 1] = torch.randn(B * S, K + 1, generator=g) * 2.0
    valid[:S] = C.valid_pattern("third", S, 1)
    if B > 1:
        valid[S:2 * S] = C.valid_pattern("ragged", S, 2)[S:]
        valid[2 * S + 64:2 * S + 128] = -1
        if S > 1300:
            valid[2 * S + 1100:2 * S + 1300] = -1
    src[valid < 0] = NAN
    for b in range(B):
        multihot[b, torch.randperm(K, generator=g)[:3 + 2 * b]] = 1
    out, info = C._settle(g, src, 1, K, rois5, valid, S, B, multihot, thr, col0, set())
    return dict(src=src, col0=col0, rois5=rois5, valid=valid, multihot=multihot, constructed=set(), ref=out, info=info, places=None)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict as weak_loss_cases.oicr_case gives it (src, col0, rois5, valid, multihot, B, S, K, mode, fg, bg, ref, info, constructed) + places"""
    mode, S, K, B, thr, seed = CASES[name]
    build = _random if mode == 1 else (_few if name == FEW else _hand)
    c = build(S, K, B, thr, seed)
    c.update(name=name, mode=mode, S=S, K=K, B=B, fg=thr[0], bg=thr[1])
    assert not C._near_thresholds(c["info"], c["valid"], S, thr[0], thr[1], c["constructed"]), name
    if mode == 1:
        assert c["info"]["gap"] >= GAP, (name, "argmax lead", c["info"]["gap"])
    return c
