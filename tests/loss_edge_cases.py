"""The catalogue of output rows at the edges of the softmax's window, the sigmoid arguments, and a net whose output rows
are WRITTEN rather than learned -- numpy only: no GPU, no library.

The training losses are built from softmax (badmaths.h:71-111: a shift that brings the row into fast_expf's domain, three
branches), fast_expf (badmaths.h:14-29: a scaling loop of 0 .. n rounds, three squarings per round), the best guess
(badmaths.h:113-141: the lowest index wins a tie), capped_log2f (charmodel-helpers.h:11-13: -100 below 1e-30) and
fast_sigmoid (badmaths.h:31-36), as oracle/recur_oracle.c states them.  A freshly initialised or a warmed-up net keeps its
outputs within a few units of zero, so none of the branches, the longer loops, the denormal likelihoods or the cap is ever
reached by training a net.  The rows here reach them by construction.

The designed net (ReLU, no bottom layer, no noise, hidden_size >= number of symbols): ih_w is zero except
ih_w[1 + hidden_size + c, 1 + c] = 1 (symbol c's input row, hidden unit c's column), ho_w is zero except
ho_w[1 + c, :] = row_c.  A stream that reads symbol c has the hidden layer bias + unit c and the output row row_c, bit for
bit under any summation order: every other product is an exact zero.

`rows` hands out finite rows only, and `checked` asserts |logit| <= 1e4 on every one of them: they go to the oracle and to
the compiled reference, whose fast_expf is badmaths.h's own -- its scaling loop does not end on an infinity (inf * 0.125
is inf), so NO test may hand the oracle or a reference binary a row that is not finite.  The library's exponential
(recur_amd/csrc/fast_exp_rule.h) is the same function on every finite float and ends on the others: an argument that is
not finite gives a quiet NaN in no rounds.  What follows from that is the library's contract (include/recur_amd.h, "Rows
that are not finite"): a softmax with an infinity or a NaN in it has no likelihoods -- every float derived from it is NaN;
its integer by-products (best guess, `correct`) are unspecified, `count` is not -- every other head, group, row, stream or
text of the same call is untouched bit for bit, and every call returns.  `nonfinite_rows` is the catalogue of such rows,
for the library alone (tests/test_fast_exp_rule.py, tests/test_gpu_nonfinite_rows.py); `fast_expf` below restates the
library's rule, which is the reference's wherever the reference returns.  `designed_nonfinite_weights` writes those rows
into a net from FINITE weights (0 * inf is NaN and would poison every stream): the poisoned symbol's hidden unit is 2, its
output weights +-2e38 where an infinity is wanted (one product overflows, under any summation order) and half the row
elsewhere; for a NaN a second unit brings -inf against +inf.
"""
import numpy as np

F = np.float32
MAX_LOGIT = 1e4
LENGTHS = (1, 2, 3, 4, 24, 42, 64, 65, 73, 128, 130, 300)  # the CPU half's; the GPU cases' lengths are among them or near
BASE_SIGMA, BASE_CLIP = 2.0, 4.5  # (clipped so that base + 45 stays below 50: the `limited` row keeps its branch at any n)


def checked(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert np.isfinite(a).all() and (np.abs(a) <= MAX_LOGIT).all(), "a logit outside [-1e4, 1e4] or not finite"
    return a


def base_row(n, seed):
    rs = np.random.default_rng([seed, n])
    return np.clip(rs.standard_normal(n) * BASE_SIGMA, -BASE_CLIP, BASE_CLIP).astype(np.float32)


def tie_placements(n):
    """(lower index, higher index) of the two equal maxima: within a lane's own values, across lanes where the lane of the
    higher index has the lower (3, 65) or the higher (5, 70) number, across the 128 a wave holds in registers"""
    p = []
    if n >= 6:
        p.append((3, n - 2))
    elif n >= 2:
        p.append((0, n - 1))
    if n > 64:
        p += [(3, 65), (5, 70)] if n > 70 else [(3, n - 1)]
    if n > 128:
        p.append((1, 129))
    return p


def rows(n, seed=0):
    """name -> float32 row of length n.  Every row starts from a seeded normal base (sigma 2), so each has several
    competing likelihoods; p and q are the two positions the special entries go to."""
    b = base_row(n, seed)
    p, q = n // 2, (n // 2 + 1) % n
    out = {}

    def put(name, row, **entries):
        row = np.array(row, np.float32)
        for pos, val in entries.values():
            row[pos] = val
        out[name] = checked(row)

    put("plain", b)
    put("at_50", b, a=(p, 50.0))
    put("above_50", b, a=(p, np.nextafter(F(50), F(np.inf))))
    put("shifted_297", b + F(297))
    put("at_m60", b, a=(p, -60.0))
    put("m61_room", b, a=(p, -61.0))
    put("limited", b + F(45), a=(p, -200.0))          # lo < -60, the shift limited by 50 - hi
    put("hi_wins", b + F(78), a=(p, -200.0))          # lo < -60 too, but hi > 50 is asked first
    put("all_m1000", np.full(n, -1000.0))
    put("all_0", np.zeros(n))
    # entries lowered by 100, 140 and 250 from near the top of a row that the shift then brings to hi = 50 (lo < -60,
    # limited): top + 5 - 100 becomes -45, a normal exponential whose quotient by the sum (>= e^50) is denormal; top - 4 -
    # 140 becomes -94, a denormal exponential; top - 250 becomes -200, an exponential that is zero
    low = b.copy()
    spots = [(p + d) % n for d in range(3)][:min(3, max(n - 1, 1))]
    top = F(np.delete(b, spots).max()) if n > 1 else F(0)
    for pos, val in zip(spots, (top + F(5 - 100), top - F(4 + 140), top - F(250))):
        low[pos] = val
    put("lowered", low)
    if n >= 2:
        put("extremes", b, a=(p, MAX_LOGIT), c=(q, -MAX_LOGIT))
    for lo_i, hi_i in tie_placements(n):
        t = b.copy()
        t[lo_i] = t[hi_i] = F(b.max() + F(1.0))
        put("tie_%d_%d" % (lo_i, hi_i), t)
    return out


def nonfinite_rows(n, seed=0):
    """name -> float32 row of length n with an infinity or a NaN in it: the same base row and the same p, q as `rows`.  For
    the library alone -- never for the oracle or a reference binary, whose exponential does not return on them.
    `pos_inf_late` (n > 64) has its infinity at n - 1: a lane's second value, the last partial float4 and, for n > 128, past
    the 128 values a wave holds in registers."""
    b = base_row(n, seed)
    p, q = n // 2, (n // 2 + 1) % n
    out = {}

    def put(name, *entries):
        row = b.copy()
        for pos, val in entries:
            row[pos] = val
        out[name] = row

    put("pos_inf", (p, np.inf))
    put("neg_inf", (p, -np.inf))
    if n >= 2:
        put("both", (p, np.inf), (q, -np.inf))
    put("nan", (p, np.nan))
    if n > 64:
        put("pos_inf_late", (n - 1, np.inf))
    return out


def arrivals(row):
    """what reaches the exponential from a row: -> (the shift's branch, the arguments row + shift); for a row of
    `nonfinite_rows` some argument is infinite -- the loop that did not end -- or, for `nan`, a NaN"""
    row = np.asarray(row, np.float32)
    adj, branch = softmax_shift(*c_extremes(row))
    with np.errstate(invalid="ignore"):
        return branch, row + adj


def sigmoid_arguments():
    g = np.linspace(-120.0, 120.0, 49).astype(np.float32)  # steps of 5: loop counts 0 (at 0) to 4
    p2 = F(0.2)
    near = [np.nextafter(p2, F(0)), p2, np.nextafter(p2, F(1))]
    x = np.concatenate([g, [700.0, -700.0, MAX_LOGIT, -MAX_LOGIT, 0.0, -0.0], near, [-v for v in near],
                        [0.1, -0.1, 1.0, -1.0, 9.0, -9.0, 90.0, -90.0, 3000.0, -3000.0, 87.5, -87.5, 88.0, -88.0]]).astype(np.float32)
    return checked(x)


# ------------------------------------------------------------------ the formulas, float32 as the C states them --

def fast_expf(x):
    """-> (values, loop counts); `fabsf(x) > 0.2` compares in double, as the C does.  An argument that is not finite is NaN in
    no rounds (fast_exp_rule.h: the reference's loop would not end on an infinity)"""
    x = np.array(x, np.float32, ndmin=1)
    count = np.zeros(x.shape, np.int64)
    finite = np.isfinite(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        while True:
            m = finite & (np.abs(x.astype(np.float64)) > 0.2)
            if not m.any():
                break
            x[m] *= F(0.125)
            count[m] += 1
        a = ((x + F(3)) * (x + F(3)) + F(3)) / ((x - F(3)) * (x - F(3)) + F(3))
        for k in range(int(count.max()) if count.size else 0):
            m = count > k
            for _ in range(3):
                a[m] = a[m] * a[m]
    a[~finite] = np.nan
    return a, count


def fast_sigmoid(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return F(1) / (F(1) + fast_expf(-np.asarray(x, np.float32) * F(1))[0])


def c_extremes(row):
    """(lo, hi) as C's comparisons find them (badmaths.h:76-80: hi = MAX(hi, x), lo = MIN(lo, x) from row[0] on, the macros
    being `hi >= x ? hi : x` and `lo < x ? lo : x`): a comparison with a NaN is false, so the NaN is taken and then given up
    for the next value -- only one at the end of the row stays.  (The device's fminf / fmaxf pass over a NaN anywhere;
    either way the NaN itself reaches the exponential and the row has no total.)"""
    row = np.asarray(row, np.float32)
    if not np.isnan(row).any():
        return row.min(), row.max()
    lo = hi = row[0]
    for x in row[1:]:
        hi = hi if hi >= x else x
        lo = lo if lo < x else x
    return lo, hi


def softmax_shift(lo, hi, mutation=None):
    lo, hi = F(lo), F(hi)
    if (hi >= F(50)) if mutation == "ge_50" else (hi > F(50)):
        return F(50) - hi, "hi"
    if lo < F(-60) and mutation != "no_lo":
        room, limit = F(-60) - lo, F(50) - hi
        if mutation == "no_min":
            return room, "room"
        return (room, "room") if room <= limit else (limit, "limited")
    return F(0), "none"


def capped_log2f(x, mutation=None):
    x = F(x)
    return F(-100) if x < (F(1e-20) if mutation == "cap_1e20" else F(1e-30)) else np.log2(x)


MUTATIONS = ("ge_50", "no_lo", "no_min", "highest_tie", "cap_1e20")


def softmax_best_guess(row, mutation=None):
    """the numpy restatement of orc_softmax_best_guess: -> (error row = -softmax, best index); `mutation` changes one rule"""
    row = np.asarray(row, np.float32)
    adj, _ = softmax_shift(*c_extremes(row), mutation=mutation)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ex, _ = fast_expf(row + adj)
        total = np.cumsum(ex, dtype=np.float32)[-1]  # in index order, as the reference's loop adds
        e = ex / total
    if mutation == "highest_tie":
        best = len(e) - 1 - int(np.argmax(e[::-1]))
    else:
        best = int(np.argmax(e))  # the first of equal maxima
    return -e, best


def scored(row, target, mutation=None):
    """what a training loss leaves for (row, target): the error row, the hit, the error on the target, the capped entropy of
    1 - error (charmodel-predict.c:302-304), and the cross entropy's capped log2 of the likelihood itself"""
    err, best = softmax_best_guess(row, mutation)
    like = -err[target]
    err = err.copy()
    with np.errstate(invalid="ignore"):
        err[target] = err[target] + F(1)
        t_err = err[target]
        entropy = capped_log2f(F(1) - t_err, mutation)
        xent = capped_log2f(like, mutation)
    return dict(error=err, hit=int(best == target), target_error=t_err, entropy=entropy, xent=xent, likelihood=like)


TINY = np.finfo(np.float32).tiny


def branch_of(row):
    """the shift branch ('none', 'hi', 'room', 'limited'), the largest fast_expf loop count, whether a likelihood is
    denormal, whether one is zero, and whether two entries tie for the best guess"""
    row = np.asarray(row, np.float32)
    adj, branch = softmax_shift(*c_extremes(row))
    _, count = fast_expf(row + adj)
    like = -softmax_best_guess(row)[0]
    return dict(branch=branch, loops=set(int(c) for c in count), denormal=bool(((like > 0) & (like < TINY)).any()),
                zero=bool((like == 0).any()), tie=bool((like == like.max()).sum() > 1))


def targets_of(row):
    """-> (kept, dropped): the arg max, the arg min, index 0 and index n - 1.  The -100 cap of the entropy statistic flips on
    one ulp where 1 - error is near 6e-8: a target is kept where 1 - error >= 1e-5 or exactly 0, dropped otherwise."""
    row = np.asarray(row, np.float32)
    want = []
    for t in (int(np.argmax(row)), int(np.argmin(row)), 0, len(row) - 1):
        if t not in want:
            want.append(t)
    kept, dropped = [], []
    for t in want:
        l = F(1) - scored(row, t)["target_error"]
        (kept if (l >= F(1e-5) or l == 0) else dropped).append(t)
    return kept, dropped


def pairs_of(named_rows):
    """[(row index, target)] over a list of (name, row), every kept target of every row; and the dropped [(name, target)]"""
    pairs, dropped = [], []
    for c, (name, row) in enumerate(named_rows):
        kept, drop = targets_of(row)
        pairs += [(c, t) for t in kept]
        dropped += [(name, len(row), t) for t in drop]
    return pairs, dropped


def coverage(named_rows, pairs=None):
    """what a set of rows scored together reaches"""
    got = dict(branches=set(), loops=set(), denormal=False, zero=False, tie=False, capped=False)
    for _, row in named_rows:
        b = branch_of(row)
        got["branches"].add(b["branch"])
        got["loops"] |= b["loops"]
        for k in ("denormal", "zero", "tie"):
            got[k] |= b[k]
    rows_ = [r for _, r in named_rows]
    for c, t in (pairs if pairs is not None else pairs_of(named_rows)[0]):
        got["capped"] |= bool(scored(rows_[c], t)["entropy"] == F(-100))
    return got


def assert_full_coverage(got, what=""):
    assert got["branches"] == {"none", "hi", "room", "limited"}, (what, got["branches"])
    assert got["loops"] >= {0, 1, 2, 3, 4}, (what, got["loops"])
    assert got["denormal"] and got["zero"] and got["capped"] and got["tie"], (what, got)


# ------------------------------------------------------------------ the designed net --

def designed_weights(I, H, O, hidden_size, symbol_rows):
    """-> (ih_w [I, H], ho_w [H, O]) of the net whose output row for symbol c is symbol_rows[c] (zeros beyond its length)"""
    assert len(symbol_rows) <= hidden_size and 1 + hidden_size + len(symbol_rows) <= I
    ih, ho = np.zeros((I, H), np.float32), np.zeros((H, O), np.float32)
    for c, row in enumerate(symbol_rows):
        assert len(row) <= O
        ih[1 + hidden_size + c, 1 + c] = 1.0
        ho[1 + c, :len(row)] = checked(row)
    return ih, ho


HUGE = F(2e38)  # twice it overflows: the one product that makes an infinity


def designed_nonfinite_weights(I, H, O, hidden_size, symbol_rows):
    """designed_weights for rows that may hold infinities and NaNs, from FINITE weights: a finite row is written as there.
    A row that is not finite gets the input weight 2 (its hidden unit is 2) and half of every finite entry (exact: asserted),
    +-2e38 where an infinity is wanted -- 2 * 2e38 overflows by itself, whatever it is added to or split from -- and for a
    NaN a spare hidden unit of its own behind the symbols', lit by the same symbol, with -2e38 against +2e38.  Every other
    stream multiplies those weights by an exact zero."""
    ih, ho = np.zeros((I, H), np.float32), np.zeros((H, O), np.float32)
    assert 1 + hidden_size + len(symbol_rows) <= I
    spare = len(symbol_rows)
    for c, row in enumerate(symbol_rows):
        row = np.asarray(row, np.float32)
        assert len(row) <= O
        fine = np.isfinite(row)
        if fine.all():
            ih[1 + hidden_size + c, 1 + c] = 1.0
            ho[1 + c, :len(row)] = checked(row)
            continue
        half = np.where(fine, row, 0) * F(0.5)
        assert np.array_equal((half * F(2)).view(np.uint32), np.where(fine, row, 0).astype(np.float32).view(np.uint32))
        half[np.isposinf(row)] = HUGE
        half[np.isneginf(row)] = -HUGE
        half[np.isnan(row)] = HUGE
        ih[1 + hidden_size + c, 1 + c] = 2.0
        ho[1 + c, :len(row)] = half
        if np.isnan(row).any():
            ih[1 + hidden_size + c, 1 + spare] = 2.0
            ho[1 + spare, :len(row)] = np.where(np.isnan(row), -HUGE, F(0))
            spare += 1
    assert spare <= hidden_size, "a NaN needs a hidden unit of its own: hidden_size >= symbols + 1 per row with one"
    assert np.isfinite(ih).all() and np.isfinite(ho).all()
    return ih, ho


def designed_forward(ih, ho, hidden_size, c):
    """the written net's answer to symbol c, float32: -> (hidden row, output row).  No recurrence is written (the hidden
    rows of ih are zero), so the input is the bias and the symbol alone; every product but the symbol's is an exact zero."""
    x = np.zeros(ih.shape[0], np.float32)
    x[0] = x[1 + hidden_size + c] = 1.0
    with np.errstate(over="ignore", invalid="ignore"):
        hid = np.maximum((x[:, None] * ih).sum(axis=0, dtype=np.float32), F(0))  # ReLU
        hid[0] = 1.0  # the bias node
        out = (hid[:, None] * ho).sum(axis=0, dtype=np.float32)
    return hid, out


def share_out(pairs, S):
    """the pairs dealt over S streams: -> [step][stream] (c, t), the last step filled up with the first pairs again"""
    steps = -(-len(pairs) // S)
    full = list(pairs) + [pairs[k % len(pairs)] for k in range(steps * S - len(pairs))]
    return [full[k * S:(k + 1) * S] for k in range(steps)]


def stream_text(pairs, S):
    """-> (text, positions): rnn_amd_set_char_step at positions[k] gives stream j the pair (c, t) = plan[k][j] -- stream j
    reads text[i + j L] and is scored against text[i + j L + 1], L = (len - 1) / S, so a stream's pairs lie at even i"""
    plan = share_out(pairs, S)
    L = 2 * len(plan)
    text = np.zeros(S * L + 1, np.uint8)
    for k, step in enumerate(plan):
        for j, (c, t) in enumerate(step):
            text[j * L + 2 * k], text[j * L + 2 * k + 1] = c, t
    assert (len(text) - 1) // S == L
    return text, [2 * k for k in range(len(plan))], plan


def ulps(a, b):
    """the distance of two float32 arrays in units in the last place (of the ordered integer line)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------ what each GPU case scores --
# (tests/test_gpu_loss_edges.py runs these; tests/test_loss_edge_rows.py asserts what they reach)

TEXT_NARROW = (42, 64)            # o_size 44 and 64: k_text_top2
TEXT_WIDE = (65, 130, 256)        # o_size 68 .. 256: k_text_top<0>
ALONE = (42, 65, 130, 300)        # k_softmax_error behind the generic output layer
HEADS = ((5, 3), (24, 4), (73, 3), (128, 2))  # (alphabet, heads): k_multi_softmax_error, in registers up to 128
GROUP_SIZES = (1, 2, 3, 7, 30)    # 43 outputs, o_size 44: k_grouped_softmax_error and k_text_top<2>
SIGMOID_WIDTH = 16                # outputs of the sigmoid cases: n = 3 and n = 16
XENT = ((42, 1), (73, 3))         # (alphabet, heads): k_xent_accumulate, k_multi_xent_accumulate


def symbol_rows(n, seed=0):
    return list(rows(n, seed).items())


def slot_rows(alen, heads, nsym):
    """[symbol][head] -> (name, row of alen): slot (c, h) holds catalogue row (c heads + h) mod the catalogue's size, from
    the next seed every time the catalogue has been walked through"""
    names = list(rows(alen, 0))
    out = []
    for c in range(nsym):
        per = []
        for h in range(heads):
            k = c * heads + h
            name = names[k % len(names)]
            per.append((name, rows(alen, k // len(names))[name]))
        out.append(per)
    return out


def head_case(alen, heads):
    """-> (symbol rows [nsym][alen heads], triples (symbol, own head, target), the slots): every catalogue row of length alen
    is some symbol's row in some head, scored as the stream's own head against each of its kept targets"""
    nsym = min(alen, 12)
    slots = slot_rows(alen, heads, nsym)
    triples = []
    for c in range(nsym):
        for h in range(heads):
            triples += [(c, h, t) for t in targets_of(slots[c][h][1])[0]]
    full = [np.concatenate([r for _, r in slots[c]]) for c in range(nsym)]
    return full, triples, slots


def group_case(nsym=16):
    """-> (symbol rows [nsym][43], offsets, sizes, the slots): group g of symbol c holds catalogue row (c + g) of its size"""
    sizes = np.array(GROUP_SIZES, np.int32)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    slots = []
    for c in range(nsym):
        per = []
        for g, n in enumerate(GROUP_SIZES):
            names = list(rows(n, 0))
            name = names[(c + g) % len(names)]
            per.append((name, rows(n, (c + g) // len(names))[name]))
        slots.append(per)
    full = [np.concatenate([r for _, r in slots[c]]) for c in range(nsym)]
    return full, offsets, sizes, slots


def group_targets(slots, step):
    """[symbol][group] targets of one step: the row's arg max, arg min, first, last in turn, -1 (not trained) now and then"""
    tg = np.zeros((len(slots), len(GROUP_SIZES)), np.int32)
    for c, per in enumerate(slots):
        for g, (_, row) in enumerate(per):
            choice = (int(np.argmax(row)), int(np.argmin(row)), 0, len(row) - 1, -1)
            tg[c, g] = choice[(step + c + 2 * g) % 5]
    return tg


def sigmoid_case(n):
    """-> symbol rows of SIGMOID_WIDTH whose first n entries are the sigmoid arguments, dealt out n per symbol"""
    x = sigmoid_arguments()
    nsym = -(-len(x) // n)
    x = np.concatenate([x, x[:nsym * n - len(x)]])
    full = np.zeros((nsym, SIGMOID_WIDTH), np.float32)
    full[:, :n] = x.reshape(nsym, n)
    full[:, n:] = np.linspace(-3, 3, SIGMOID_WIDTH - n, dtype=np.float32)[None, :] if n < SIGMOID_WIDTH else 0
    return [checked(r) for r in full]


def xent_safe(like):
    """capped_log2f's own threshold flips on one ulp near 1e-30: a scored likelihood lies a factor of 10 off it"""
    return like >= F(1e-29) or like < F(1e-31)


def xent_case(alen, heads):
    """-> (symbol rows [alen][alen heads], text, the slots, dropped): every symbol of the alphabet has a row of catalogue
    rows; the text walks every symbol and, behind it, each of its targets -- a target is the next step's input, so the
    pairs (target, next symbol) are scored as well.  A target whose likelihood is not xent_safe in every head is dropped
    (and listed); where the step from a target to the next symbol is not, a symbol that is safe on both sides goes between."""
    slots = slot_rows(alen, heads, alen)
    full = [np.concatenate([r for _, r in slots[c]]) for c in range(alen)]
    like = [[-softmax_best_guess(row)[0] for _, row in slots[c]] for c in range(alen)]

    def safe(a, b):
        return all(xent_safe(l[b]) for l in like[a])

    text, dropped = [], []
    for c in range(alen):
        want = []
        for _, row in slots[c]:
            for t in (int(np.argmax(row)), int(np.argmin(row)), 0, alen - 1):
                if t not in want:
                    want.append(t)
        for t in want[:4 + heads]:
            if not safe(c, t):
                dropped.append((c, t))
                continue
            if text and not safe(text[-1], c):
                text.append(next(b for b in range(alen) if safe(text[-1], b) and safe(b, c)))
            text += [c, t]
    return full, np.array(text, np.uint8), slots, dropped


def xent_scored(slots, text, skip=0):
    """[(head, name, row, target)] of every scored step of the text"""
    out = []
    for i in range(skip, len(text) - 1):
        for h, (name, row) in enumerate(slots[text[i]]):
            out.append((h, name, row, int(text[i + 1])))
    return out
