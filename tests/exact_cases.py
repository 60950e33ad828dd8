"""The catalogue of EXACT nets: nets that are written, not learned, so that every sum of a training generation is a sum of
small integers times a power of two and is therefore the same float32 in any order.  The catalogue and the restatement are
numpy only (no GPU, no library); `OracleSide` at the end drives oracle/liboracle.so through the same steps.

The parity tests compare "at the bar" (1e-4 of each array's largest element), which is right for random data, where the
device and the reference add in different orders, and blind to anything smaller: one K element left out of one chain step,
one stream's deepest step missing from a weight delta, a K-split plane added twice at a tile edge.  On the nets below no
order can round, so the device owes the oracle every element of every array EXACTLY (tests/test_gpu_exact_generations.py),
whatever tile, K split, plane count or launch form the plans picked.  tests/test_exact_cases_cpu.py shows from the oracle
alone that the premise holds.

Two constructions, each a pure function of (shape, seed):

(a) `dyadic_net` with caller-written error rows (`error_rows`).  W_ih: every hidden column gets +1 from one hidden row, -1
    from another, a bias in {-1, 0, 1} and two input rows in {-2 .. 2} \\ {0}; column 0 and the pad columns are zero.  W_ho:
    integers in {-1, 0, 1}, about half of them zero, two columns all zero.  Inputs are one-hot or dense integers 0 .. 1.
    Hidden values are then small integers, many exactly 0 and, under RECLIP20, some exactly 20: both gates are exercised
    exactly.  Error rows are integers in {-2 .. 2} times 2^-10; per generation one stream's row is all zero (its hidden error
    is exactly 0: the loop ends before its first step) and one stream's row is non-zero only on outputs whose W_ho column
    is zero (a top delta without a hidden error).  (`steep`: every so-many-th column takes +3 instead of +1 -- at depth 3
    the ring is full after six generations, in which +1 and one input can bring no unit to 20.)
(b) `zero_answer_net`, for the calls that compute their own loss.  Hidden units come in pairs (2i + 1, 2i + 2) with
    identical W_ih columns whose own rows feed every other unit identically, so the two are equal in every stream, forever;
    W_ho's row of the second is minus the first's, entries in {-1, 0, 1} times 2^-8.  Every output is exactly 0,
    fast_expf(0) is exactly 1 ((9 + 3) / (9 + 3)), a softmax over 2^k outputs is exactly 2^-k, fast_sigmoid(0) exactly 1/2:
    o_error is dyadic for every loss, and the hidden error W_ho[y, target] - mean_x W_ho[y, x] is not zero.  The pairs
    diverge at the first update: exact for ONE training generation and the forward pass after it.  What the construction
    costs: twins have identical W_ih columns and opposite hidden errors, so the error the FIRST chain step hands down
    cancels to exactly 0 and the chain ends there (depth 0 on every stream).  These cases hold the loss kernels, the top
    backprop, the top delta, the newest step's recurrent delta and the update; the chain's deeper steps are (a)'s.

Scalars: learn_rate 2^-6, momentum 1/2, momentum_weight 1/2, ho_scale 1/2 or 2, momentum arrays on a 2^-10 grid and not
zero.  Rules that divide or take roots (SIMPLIFIED_NESTEROV, ADAGRAD, ADADELTA, RPROP, RESQRT) are out: they round.

`Restated` is the generation in numpy float64: the forward pass, the output layer, the top backprop (plain and ranged, with
the reference's stale entries), every chain step with the ping-pong of the two error vectors, both deltas and the update.
Every sum of products it forms goes through `Budget.dot`, which checks the CONDITION under which no order can round: the
operands are integers times the case's design grids 2^-ka and 2^-kb, and (|A| @ |B|).max() 2^(ka + kb) <= 2^23 -- every
partial sum in any order is then an integer of at most 24 bits times the grid; 2^23 keeps one spare bit.

What the condition does NOT give, and the tests therefore hold at the bar instead: after the update the weights sit on a
grid of about 2^-17, so the forward pass behind it has exact hidden rows (small integers times that grid) but an output
layer whose products lie on the product of two such grids -- `FORWARD_AFTER` names the stages and `budget` reports which
of them fit.  A second training generation is out of reach altogether.  The loss statistics use logarithms.

The scalars the chain decides by (its three thresholds, min_error_factor's step) are single float32 operations on exact
inputs: the restatement forms them with float32 operands, as the C does.
"""
import numpy as np

F = np.float32
RELU, RECLIP20 = 1, 5
WEIGHTED, NESTEROV, CLASSICAL = 0, 1, 3
ERR_GRID = 10          # error rows: integers times 2^-10
MOM_GRID = 10          # momentum arrays at the start
ZERO_W_GRID = 8        # W_ho of the zero-answer nets
LEARN_RATE = 2.0 ** -6
MOMENTUM = 0.5
MOMENTUM_WEIGHT = 0.5
LIMIT_BITS = 23


def padded(input_size, hidden_size, output_size):
    return (hidden_size + input_size + 1 + 3) & ~3, (hidden_size + 1 + 3) & ~3, (output_size + 3) & ~3


# ------------------------------------------------------------------------------------------- the cases --
# kind "dyadic": separate calls (advance, opinion, put_o_error, calc_deltas, apply_learning); the others are zero-answer
# cases named after the call that computes their loss.

def _c(kind, input_size, hidden_size, output_size, S, D, **more):
    c = dict(kind=kind, input_size=input_size, hidden_size=hidden_size, output_size=output_size, S=S, D=D, activation=RELU,
             one_hot=True, as_floats=False, method=WEIGHTED, ho_scale=0.5, seed=11, api="batched", ranges=None, masked=False, steep=0)
    c.update(more)
    return c


# what the plans must give a case in lock step (tests/test_exact_cases_cpu.py asks calc_plan.h, chain_plan.h and fwd_plan.h
# through their harnesses): "calc" for both forms of the deltas call, "planes" / "summed" for one of them
#   (rnn_amd_set_calc_deltas: accumulate 0 leaves the sums as planes in the engine's own workspace of 8 I H + 64 x 128 H
#   floats, accumulate 1 sums at once; the per-net call and the text step pass no workspace of their own)
TOP_DONE = 0x40000000  # RAMD_TOP_DONE: the text step has done the top backprop with the loss
HEADS = 0x10000000     # RAMD_RANGES_ARE_HEADS: one range list per stream, heads of at least 24 columns

# (the step sizes its workspace for the heads' partial products -- streams x heads x H floats -- on first use, and
# announces its update: the deltas are left as planes in the engine's own workspace)
HEADS_FORMS = dict(calc=dict(top="sparse", ho_gemm="heads", small=0, direct=0, dma=0),
                   calc_args=dict(flags=HEADS, ranges=1, range_stride=132, mheads_alen=32, mheads_part_floats=6 * 2 * 44,
                                  fuse_want=0, own_slab_floats=8 * 76 * 44 + 64 * 128 * 44),
                   fwd=dict(hidden="gemm", output="rows"), fwd_args=dict(mode=1, advance=1, want=0))

CASES = {
    # k_fwd_small, k_bptt_small: one net through the per-net calls
    "per-net": _c("dyadic", 10, 31, 5, 1, 4, api="per-net", one_hot=False, method=CLASSICAL, ho_scale=2.0,
                  forms=dict(calc=dict(small=1), fwd=dict(hidden="small"), fwd_args=dict(one_net=1, mode=0))),
    # the generic forward GEMM, k_chain_main with the stages counted at run time (ns 0), dense extras, k_gemm deltas in
    # 64 x 64 tiles with a 6-way K split, units at 20.0
    "ragged": _c("dyadic", 10, 40, 16, 6, 6, activation=RECLIP20, one_hot=False, method=NESTEROV, seed=5,
                 forms=dict(calc=dict(direct=0, dma=0, small=0, big=0, ks=6, extras="dense", top="plain"),
                            planes=dict(ho_gemm="planes"), summed=dict(ho_gemm="summed"), calc_args=dict(dense_inputs=1),
                            chain=dict(wanted=0, form="main", ns=0), fwd=dict(hidden="gemm"))),
    # the same net with error ranges and an active mask: k_top_backprop_ranged with 16 partial sums per stream,
    # k_top_backprop_scale
    "ranged": _c("dyadic", 10, 40, 16, 6, 6, activation=RECLIP20, one_hot=False, ranges=((4, 4), (9, 3)), masked=True, seed=5,
                 forms=dict(calc=dict(direct=0, dma=0, small=0, top="ranged", top_nb=16, ho_gemm="summed"),
                            calc_args=dict(dense_inputs=1, ranges=1, active=1),
                            chain=dict(wanted=0, form="main", ns=0), fwd=dict(hidden="gemm"))),
    # k_fwd_fused, the one-launch chain in 16-stream tiles (the dense extras in k_extras_dense), k_delta_dma with its rest rows by
    # the generic kernel, the top delta paired with them.  (The one-hot rows are fed as floats: the one-hot call without an
    # advance of its own gets the generic forward GEMM, which "h1024" and "wide" run.)
    "h256": _c("dyadic", 32, 256, 32, 32, 5, ho_scale=2.0, as_floats=True,
               forms=dict(calc=dict(direct=0, dma=1, has_rest=1, extras="dense"), planes=dict(ho_gemm="planes_paired"),
                          summed=dict(ho_gemm="paired_summed"), calc_args=dict(dense_inputs=1),
                          chain=dict(wanted=1, uniform=1, seg0="0,32,1,0,32,0>240,1"), fwd=dict(hidden="fused"))),
    # dense extras inside the chain launch, k_delta_direct with a 4-way K split, its planes left for the update (here every
    # step's snapshot sums them with k_delta_finalize; tests/settle_cases.py is where k_apply does)
    "h512": _c("dyadic", 16, 512, 16, 128, 5, one_hot=False,
               forms=dict(calc=dict(direct=1, direct_runs=1, dks=4, xc_req="dense"), planes=dict(ho_gemm="planes_paired"),
                          summed=dict(ho_gemm="paired_summed"), calc_args=dict(dense_inputs=1),
                          chain=dict(wanted=1, uniform=1, seg0="0,128,1,0,128,0>128,1"), fwd=dict(hidden="fused"))),
    # the one-launch chain in 32-stream tiles, k_delta_direct in whole rounds (no K split), the gathered one-hot extras
    "h1024": _c("dyadic", 32, 1024, 32, 160, 5,
                forms=dict(calc=dict(direct=1, direct_runs=1, dks=1, xc_req="gather"),
                           chain=dict(wanted=1, uniform=1, seg0="0,160,0,0,160,0>256,0"), fwd=dict(hidden="gemm"))),
    # k_chain_wide, k_gemm2 (128 x 128 tiles; RECLIP20 keeps k_delta_dma out, which every shape of k_chain_wide would get)
    "wide": _c("dyadic", 32, 1536, 32, 384, 3, activation=RECLIP20, steep=8,
               forms=dict(calc=dict(direct=0, dma=0, big=1, ks=3), chain=dict(form="wide", ns=24), fwd=dict(hidden="gemm"))),
    # rnn_amd_set_char_step: k_text_top2 bit for bit, the top delta asked of the chain launch
    "text": _c("text", 32, 256, 32, 32, 5,
               forms=dict(calc=dict(top="done", ho_asked=1, dma=1), calc_args=dict(flags=TOP_DONE),
                          chain=dict(wanted=1, uniform=1), fwd=dict(hidden="fused", end="left"),
                          fwd_args=dict(mode=3, advance=1, want=1))),
    # the benchmark's path: update and top delta in k_delta_direct's own launch
    "text, full": _c("text", 32, 1024, 32, 256, 5,
                     forms=dict(calc=dict(top="done", direct=1, direct_runs=1, direct_fuse=1, ho_in_delta=1),
                                calc_args=dict(flags=TOP_DONE), chain=dict(wanted=1, uniform=1),
                                fwd=dict(hidden="fused", end="left"), fwd_args=dict(mode=3, advance=1, want=1))),
    # rnn_amd_set_dense_step_sigmoid_mse: k_text_top<1>, the 4-column output form; targets in {0, 1/4, 1}
    "sigmoid": _c("sigmoid", 9, 64, 3, 64, 4, one_hot=False,
                  forms=dict(calc=dict(top="done"), calc_args=dict(flags=TOP_DONE, dense_inputs=1, accumulate=1),
                             fwd=dict(hidden="fused", end="left"), fwd_args=dict(mode=2, want=2))),
    # rnn_amd_set_opinion_grouped_softmax + rnn_amd_set_calc_deltas with `trained` as the mask + rnn_apply_learning:
    # k_text_top<2>, the active mask; groups of 2, 4 and 8, a third of the streams untrained, error weights 1/2, 1, 2
    "groups": _c("groups", 12, 64, 14, 12, 4, one_hot=False, method=NESTEROV, ho_scale=2.0,
                 forms=dict(calc=dict(top="done"), calc_args=dict(flags=TOP_DONE, dense_inputs=1, accumulate=1, active=1, defer=0),
                            fwd=dict(hidden="fused", end="left"), fwd_args=dict(mode=2, want=2))),
    # rnn_amd_set_char_step_fused: one net, batch 1: the top layer's update at once, without ho_scale or a top delta, and
    # the recurrent layer's behind the chain (k_fused_updates)
    "fused single": _c("fused", 32, 64, 32, 1, 4, seed=12,
                       forms=dict(calc=dict(top="done", small=1), calc_args=dict(flags=TOP_DONE, defer=0),
                                  fwd=dict(hidden="fused", end="left"), fwd_args=dict(mode=3, advance=1, want=1))),
    # rnn_amd_set_multi_step: k_multi_softmax_error, k_top_heads_partial / _combine, k_ho_delta_heads; two heads of 32
    # symbols, the own head alone (leakage 0) ...
    "heads": _c("heads", 32, 40, 64, 6, 6, leakage=0.0, seed=17,
                forms=HEADS_FORMS),
    # ... and every head (leakage 1 -- as the largest float below it: the reference's `leakage * UINT64_MAX` does not fit
    # its integer at 1.0 itself), which is one merged range of 64 columns and one draw per stream
    "heads, leaked": _c("heads", 32, 40, 64, 6, 6, seed=17, leakage=float(np.nextafter(F(1), F(0))),
                        forms=HEADS_FORMS),
}
DYADIC = [k for k, c in CASES.items() if c["kind"] == "dyadic"]
ZERO_ANSWER = [k for k, c in CASES.items() if c["kind"] != "dyadic"]


def generations(c):
    """delta generations of a dyadic case: every ring position is the newest once, and three more"""
    return c["D"] + 3


def accumulates(c, g):
    """generations alternate between the two forms of rnn_amd_set_calc_deltas: accumulate 1 (the sums, added to what is
    there) and 0 (the deltas left as planes for the update to add up); the last one in front of the update is a 0"""
    return (generations(c) - 1 - g) % 2


# ------------------------------------------------------------------------------------- construction (a) --

def dyadic_net(c):
    """-> dict(ih_w, ho_w, ih_m, ho_m, zero_cols): the written net of a case and its momentum arrays at the start"""
    hs, isz, osz = c["hidden_size"], c["input_size"], c["output_size"]
    I, H, O = padded(isz, hs, osz)
    rs = np.random.default_rng([c["seed"], hs, isz, osz])
    ih, ho = np.zeros((I, H)), np.zeros((H, O))
    off = hs + 1
    for x in range(1, hs + 1):
        a, b = rs.choice(hs, 2, replace=False) + 1
        ih[a, x], ih[b, x] = 1, -1
        if c["steep"] and x % c["steep"] == 0:
            ih[a, x] = 3
        ih[0, x] = rs.integers(-1, 2)
        for r in rs.choice(isz, 2, replace=False):
            ih[off + r, x] = rs.choice([-2, -1, 1, 2])
    ho[:hs + 1, :osz] = rs.integers(-1, 2, (hs + 1, osz)) * (rs.random((hs + 1, osz)) < 0.75)
    zero_cols = (1, osz - 1)
    ho[:, zero_cols] = 0
    m = {}
    for k, w, live in (("ih_m", ih, (slice(0, off + isz), slice(1, hs + 1))), ("ho_m", ho, (slice(0, hs + 1), slice(0, osz)))):
        m[k] = np.zeros(w.shape)
        g = rs.integers(-3, 4, w.shape)
        g[g == 0] = 1
        m[k][live] = g[live] * 2.0 ** -MOM_GRID
    return dict(ih_w=ih, ho_w=ho, zero_cols=zero_cols, **m)


def inputs_of(c, g):
    """generation g's inputs: -> hot [S] (one-hot cases) or x [S][input_size] of integers 0 .. 1"""
    rs = np.random.default_rng([c["seed"], 1000 + g])
    if c["one_hot"]:
        return rs.integers(0, c["input_size"], c["S"]).astype(np.int32)
    return rs.integers(0, 2, (c["S"], c["input_size"])).astype(np.float32)


def fed(c, x):
    """the inputs as a library is given them: hot [S], or rows of floats (dense inputs, or one-hot rows `as_floats`)"""
    if np.ndim(x) == 2 or not c["as_floats"]:
        return x
    rows = np.zeros((c["S"], c["input_size"]), np.float32)
    rows[np.arange(c["S"]), x] = 1
    return rows


def plan_args(c, form):
    """the arguments of the three plan harnesses for a case; form: "planes" or "summed" """
    I, H, _ = padded(c["input_size"], c["hidden_size"], c["output_size"])
    shape = dict(input=c["input_size"], hidden=c["hidden_size"], output=c["output_size"], streams=c["S"])
    calc = dict(shape, depth=c["D"], activation=c["activation"])
    if c["kind"] == "dyadic":
        calc.update(accumulate=int(form == "summed"), defer=int(form == "planes" and c["api"] == "batched"))
        if calc["defer"]:
            calc["own_slab_floats"] = 8 * I * H + 64 * 128 * H
    calc.update(c["forms"].get("calc_args", {}))
    fwd = dict(shape, mode=1 if c["one_hot"] and not c["as_floats"] else 2, advance=0, want=0)
    fwd.update(c["forms"].get("fwd_args", {}))
    return calc, dict(hidden=c["hidden_size"], nrows=c["S"], depth=c["D"]), fwd


def row_kind(c, g, s):
    """0: the all-zero row; 1: non-zero only where W_ho's column is zero; else an ordinary row.  The two special rows walk
    through the streams (through the generations, where there is one stream)"""
    return (s + g) % max(c["S"], 4)


def error_rows(c, g, zero_cols):
    """generation g's error rows [S][O]: integers in {-2 .. 2} times 2^-10 on the real outputs (inside the ranges, where
    the case has ranges)"""
    S, osz = c["S"], c["output_size"]
    O = padded(c["input_size"], c["hidden_size"], osz)[2]
    rs = np.random.default_rng([c["seed"], 2000 + g])
    e = np.zeros((S, O))
    e[:, :osz] = rs.integers(-2, 3, (S, osz))
    if c["ranges"]:
        inside = np.zeros(O, bool)
        for start, n in c["ranges"]:
            inside[start:start + n] = True
        e[:, ~inside] = 0
    for s in range(S):
        k = row_kind(c, g, s)
        if k == 0:
            e[s] = 0
        elif k == 1 and not c["ranges"]:
            keep = np.zeros(O, bool)
            keep[list(zero_cols)] = True
            e[s, ~keep] = 0
            e[s, zero_cols[0]] = 2
    return (e * 2.0 ** -ERR_GRID).astype(np.float32)


def active_mask(c, g):
    """the streams rnn_amd_set_calc_deltas is asked for: all, or (masked cases) all but two that walk; stream 0 stays"""
    a = np.ones(c["S"], np.uint8)
    if c["masked"]:
        first = 2 + g % (c["S"] - 3)
        a[[first, first + 1]] = 0
    return a


def range_pairs(c):
    """the case's error ranges as the flat list of (start, len) pairs the libraries take, closed by (-1, 0)"""
    return None if not c["ranges"] else [v for p in c["ranges"] for v in p] + [-1, 0]


# ------------------------------------------------------------------------------------- construction (b) --

def zero_answer_net(c):
    """-> dict(ih_w, ho_w, ih_m, ho_m): units 2i + 1 and 2i + 2 are twins; W_ho's rows of a pair cancel"""
    hs, isz, osz = c["hidden_size"], c["input_size"], c["output_size"]
    assert hs % 2 == 0
    I, H, O = padded(isz, hs, osz)
    rs = np.random.default_rng([c["seed"], hs, isz, osz, 7])
    ih, ho = np.zeros((I, H)), np.zeros((H, O))
    off, pairs = hs + 1, hs // 2
    for p in range(pairs):
        col = np.zeros(I)
        a, b = rs.choice(pairs, 2, replace=False)
        col[1 + 2 * a], col[2 + 2 * b] = 1, -1    # (either unit of a pair speaks for both: they are equal)
        col[0] = rs.integers(-1, 2)
        for r in rs.choice(isz, 2, replace=False):
            col[off + r] = rs.choice([-2, -1, 1, 2])
        ih[:, 1 + 2 * p] = ih[:, 2 + 2 * p] = col
        row = rs.integers(-1, 2, osz) * 2.0 ** -ZERO_W_GRID
        if not row.any():
            row[p % osz] = 2.0 ** -ZERO_W_GRID
        ho[1 + 2 * p, :osz], ho[2 + 2 * p, :osz] = row, -row
    m = {}
    for k, w, live in (("ih_m", ih, (slice(0, off + isz), slice(1, hs + 1))), ("ho_m", ho, (slice(0, hs + 1), slice(0, osz)))):
        m[k] = np.zeros(w.shape)
        g = rs.integers(-3, 4, w.shape)
        g[g == 0] = 1
        m[k][live] = g[live] * 2.0 ** -MOM_GRID
    return dict(ih_w=ih, ho_w=ho, **m)


def text_of(c):
    """a text for rnn_amd_set_char_step: every symbol of the alphabet, seeded"""
    rs = np.random.default_rng([c["seed"], 3000])
    return rs.integers(0, c["input_size"], c["S"] * 24 + 1).astype(np.uint8)


def text_taps(text, i, S):
    """the streams' symbols and targets in generation i (charmodel-predict.c:288-300)"""
    L = len(text)
    off = (i + np.arange(S) * ((L - 1) // S)) % (L - 1)
    return text[off].astype(np.int32), text[off + 1].astype(np.int32)


def sigmoid_targets(c, g):
    """[S][n] targets in {0, 1/4, 1}: the error 1/4 (t - 1/2) is dyadic"""
    rs = np.random.default_rng([c["seed"], 4000 + g])
    return rs.choice(np.array([0.0, 0.25, 1.0], np.float32), (c["S"], c["output_size"]))


GROUP_SIZES = (2, 4, 8)


def group_layout():
    sizes = np.array(GROUP_SIZES, np.int32)
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32), sizes


def group_targets(c, g):
    """[S][groups]: every third stream has nothing to train (-1 throughout), every third leaves one group out"""
    rs = np.random.default_rng([c["seed"], 5000 + g])
    t = np.stack([rs.integers(0, n, c["S"]) for n in GROUP_SIZES], axis=1).astype(np.int32)
    for s in range(c["S"]):
        if s % 3 == 0:
            t[s] = -1
        elif s % 3 == 1:
            t[s, (s // 3) % len(GROUP_SIZES)] = -1
    return t


def group_weights(c):
    """error_weight per output: 1/2, 1 or 2"""
    rs = np.random.default_rng([c["seed"], 6000])
    O = padded(c["input_size"], c["hidden_size"], c["output_size"])[2]
    return rs.choice(np.array([0.5, 1.0, 2.0], np.float32), O)


def group_errors(c, g):
    """-> (o_error [S][O] of answers that are all 0: weight (onehot - 1 / n) per trained group, trained [S], groups, wins,
    wrongness): the winner among equal answers is the lowest index"""
    goff, gsize = group_layout()
    t, w = group_targets(c, g), group_weights(c).astype(np.float64)
    O = len(w)
    e = np.zeros((c["S"], O))
    groups = wins = 0
    wrong = 0.0
    for s in range(c["S"]):
        for i, (o, n) in enumerate(zip(goff, gsize)):
            if t[s, i] >= 0:
                e[s, o:o + n] = -1.0 / n
                e[s, o + t[s, i]] += 1
                groups, wins, wrong = groups + 1, wins + int(t[s, i] == 0), wrong + 1 - 1.0 / n
        if (t[s] >= 0).any():
            e[s, :c["output_size"]] *= w[:c["output_size"]]
    return e, (t >= 0).any(axis=1).astype(np.uint8), groups, wins, wrong


def head_inputs(c, g):
    """-> (hot [S], next [S], the own head [S]) of a multi-head step over heads of input_size symbols"""
    rs = np.random.default_rng([c["seed"], 7000 + g])
    A, S = c["input_size"], c["S"]
    return (rs.integers(0, A, S).astype(np.int32), rs.integers(0, A, S).astype(np.int32),
            rs.integers(0, c["output_size"] // A, S).astype(np.int32))


def head_errors(c, g):
    """-> (o_error [S][O] of answers that are all 0, the trained columns [S][O]): the own head, or every head"""
    A, S = c["input_size"], c["S"]
    heads = c["output_size"] // A
    O = padded(A, c["hidden_size"], c["output_size"])[2]
    _, nxt, cls = head_inputs(c, g)
    e, cols = np.zeros((S, O)), np.zeros((S, O), bool)
    for s in range(S):
        for h in range(heads):
            if h == cls[s] or c["leakage"] > 0:
                e[s, h * A:(h + 1) * A] = -1.0 / A
                e[s, h * A + nxt[s]] += 1
                cols[s, h * A:(h + 1) * A] = True
    return e, cols


def net_of(c):
    return dyadic_net(c) if c["kind"] == "dyadic" else zero_answer_net(c)


# ------------------------------------------------------------------------------------------ the budget --

class Budget:
    """Every sum of products of the restatement passes through `dot`.  The condition: A 2^ka and B 2^kb are integers and
    (|A| @ |B|).max() 2^(ka + kb) <= 2^23.  The grid of an operand is the smallest that holds it, found from the operand --
    a design grid is a property of the numbers, and finding it states no more than checking it -- and capped at 40."""

    def __init__(self):
        self.bits, self.failed = {}, []

    @staticmethod
    def grid(a):
        a = np.abs(np.asarray(a, np.float64))
        a = a[a != 0]
        if not a.size:
            return 0
        k = 0
        while k <= 40:
            v = a * 2.0 ** k
            if np.array_equal(v, np.rint(v)):
                return k
            k += 1
        return None

    def note(self, stage, A, B, largest):
        ka, kb = self.grid(A), self.grid(B)
        if ka is None or kb is None:
            self.failed.append("%s: an operand is on no dyadic grid" % stage)
            return
        bits = (np.log2(largest) if largest > 0 else 0.0) + ka + kb
        self.bits[stage] = max(self.bits.get(stage, 0.0), float(bits))

    def dot(self, stage, A, B):
        self.note(stage, A, B, float((np.abs(A) @ np.abs(B)).max(initial=0.0)))
        return A @ B

    def total(self, stage, A, B, abs_sum):
        """a sum built up over several dots (a delta over streams, steps and generations): abs_sum is its sum of |terms|"""
        self.note(stage, A, B, float(np.max(abs_sum, initial=0.0)))

    def over(self, stages=None):
        return sorted(k for k, b in self.bits.items() if b > LIMIT_BITS and (stages is None or k in stages)) + self.failed


class NoBudget:
    """the restatement without the book-keeping (half the matrix products)"""
    bits = {}

    def dot(self, stage, A, B):
        return A @ B

    def total(self, *a):
        pass


# stages of the forward pass behind the update, whose weights sit on a fine grid: reported, and exact only where they fit
FORWARD_AFTER = ("hidden after", "output after")
GENERATION = ("hidden", "output", "top backprop", "chain", "error sum", "ih_delta", "ho_delta", "update")


# ------------------------------------------------------------------------------------- the restatement --

MUTATIONS = ("deepest_step_not_added", "last_column_left_out", "stream_left_out_of_ho_delta", "clipped_unit_live",
             "zero_row_runs_deeper", "column_0_not_cleared")


class Restated:
    """A training set of S streams in float64, in the layout of the oracle's arrays.  `mutation` breaks one rule."""

    def __init__(self, c, net=None, mutation=None, budget=None):
        self.c, self.mutation = c, mutation
        self.budget = budget or NoBudget()
        self.tracked = budget is not None
        hs, isz, osz = c["hidden_size"], c["input_size"], c["output_size"]
        self.S, self.D = S, D = c["S"], c["D"]
        self.I, self.H, self.O = I, H, O = padded(isz, hs, osz)
        net = net or net_of(c)
        self.ih_w, self.ho_w = net["ih_w"].copy(), net["ho_w"].copy()
        self.ih_m, self.ho_m = net["ih_m"].copy(), net["ho_m"].copy()
        self.ih_delta, self.ho_delta = np.zeros((I, H)), np.zeros((H, O))
        self.ih_abs, self.ho_abs = np.zeros((I, H)), np.zeros((H, O))
        self.hist = np.zeros((D, S, I))
        self.hidden, self.output, self.o_error = np.zeros((S, H)), np.zeros((S, O)), np.zeros((S, O))
        self.err_a, self.err_b = np.zeros((S, I)), np.zeros((S, I))
        self.index = np.full(S, 1 if D > 1 else 0, np.int32)
        self.mef = np.full(S, F(1e-12) * F(H), np.float32)
        self.ih_scale = np.ones(S, np.float32)
        self.depth = np.zeros(S, np.int32)
        self.generation = np.zeros(S, np.uint32)
        self.top_raw, self.top_scaled = np.zeros(S), np.zeros(S)
        self.margins = []   # (stream, step, error_sum, ceiling, exit threshold, give-up threshold) of every executed step
        self.finals = []    # (stream, the last executed step's error_sum, ceiling): what ih_scale is decided by

    # -- forward --
    def advance(self):
        self.index = (self.index + 1) % self.D

    def opinion(self, x, stage="hidden"):
        """x: hot [S] or dense [S][input_size]"""
        c, S, off = self.c, self.S, self.c["hidden_size"] + 1
        slot = self.hist[self.index, np.arange(S)]
        x = np.asarray(x)
        if x.ndim == 1:
            slot[:, off:off + c["input_size"]] = 0
            slot[np.arange(S), off + x] = 1
        else:
            slot[:, off:off + c["input_size"]] = x
        slot[:, :off] = self.hidden[:, :off]
        slot[:, 0] = 1
        assert (slot.sum(axis=1) <= 16.0 * self.I).all(), "the input clip is not part of the construction"
        self.hist[self.index, np.arange(S)] = slot
        hid = self.budget.dot(stage, slot, self.ih_w)
        live = hid[:, 1:]
        if c["activation"] == RECLIP20:
            live = np.minimum(live, 20.0)
        hid[:, 1:] = np.maximum(live, 0.0)
        hid[:, 0] = 1
        self.hidden = hid
        self.output = self.budget.dot("output" + stage[6:], hid, self.ho_w)

    # -- backward --
    def calc_deltas(self, accumulate, ranges=None, active=None, stream_cols=None, fused=False):
        """ranges: the error ranges every stream shares; stream_cols [S][O]: one contiguous range per stream instead;
        fused: rnn_bptt_calculate's order -- the top layer is updated at once (the plain rate, no delta kept), the
        recurrent layer's update follows the chain"""
        c, b, S, I, H, O, D = self.c, self.budget, self.S, self.I, self.H, self.O, self.D
        streams = [s for s in range(S) if active is None or active[s]]
        if not accumulate:
            self.ho_delta[:], self.ho_abs[:], self.ih_delta[:], self.ih_abs[:] = 0, 0, 0, 0
        on = np.zeros(S, bool)
        on[streams] = True
        # the top backprop
        unit = self.hidden != 0
        unit[:, 0] = False
        if stream_cols is not None:
            e = b.dot("top backprop", self.o_error * stream_cols, self.ho_w.T) * unit
            top = np.abs(e).sum(axis=1)
            self.err_a[:, :H] = np.where(on[:, None] & unit, e, self.err_a[:, :H])
        elif ranges is None:
            e = b.dot("top backprop", self.o_error, self.ho_w.T) * unit
            top = np.abs(e).sum(axis=1)
            self.err_a[on, 1:H] = e[on, 1:]
        else:
            e, top = np.zeros((S, H)), np.zeros(S)
            for start, n in ranges:
                lo, hi = start & ~3, (start & ~3) + ((n + 3) & ~3)
                e = e + b.dot("top backprop", self.o_error[:, lo:hi], self.ho_w[:, lo:hi].T) * unit
                top = top + np.abs(e).sum(axis=1)     # (|e| is added once per range while e keeps running)
            keep = on[:, None] & unit                 # (an inactive unit keeps last time's entry)
            self.err_a[:, :H] = np.where(keep, e, self.err_a[:, :H])
        assert (top[on] <= 2.0 * H).all(), "the top error's clip is not part of the construction"
        self.top_raw[on], self.top_scaled[on] = top[on], top[on]
        # the top delta
        cols = np.zeros(O, bool)
        if ranges is None:
            cols[:] = True
        else:
            for start, n in ranges:
                cols[start & ~3:(start & ~3) + ((n + 3) & ~3)] = True
        oe = self.o_error * (cols if stream_cols is None else stream_cols) * on[:, None]
        if self.mutation == "stream_left_out_of_ho_delta" and oe.any():
            oe[np.nonzero(oe.any(axis=1))[0][-1]] = 0    # (the last stream that has anything to add)
        if fused:
            self._update(self.ho_w, b.dot("ho_delta", self.hidden.T, oe), self.ho_m, LEARN_RATE, WEIGHTED)
        else:
            self.ho_delta += b.dot("ho_delta", self.hidden.T, oe)
        if self.tracked:
            self.ho_abs += np.abs(self.hidden.T) @ np.abs(oe)
        b.total("ho_delta", self.hidden, oe, self.ho_abs)
        # the chain
        top32 = top.astype(np.float32)
        max_sum, ceiling, gain = F(2) * top32 + F(1), top32, F(1e-8) * top32
        low = np.minimum(self.mef / F(LEARN_RATE), gain)
        running = on.copy()
        a_is_h = np.ones(S, bool)          # which of the two vectors is h_error
        err_sum = np.zeros(S)
        t_left = np.full(S, D)
        self.ran = np.zeros((S, D), bool)
        offset = self.index.copy()
        off = c["hidden_size"] + 1
        for step in range(D):
            h = np.where(a_is_h[:, None], self.err_a, self.err_b)
            if self.mutation != "column_0_not_cleared":
                h[:, 0] = 0
            h[:, off:H] = 0
            x = self.hist[offset, np.arange(S)]
            live = x != 0
            if c["activation"] == RECLIP20 and self.mutation != "clipped_unit_live":
                live &= x < 20.0
            xl = x * live * running[:, None]
            hh = h[:, :H] * running[:, None]
            if self.mutation == "deepest_step_not_added" and step == D - 1 and running.any():
                xl[np.nonzero(running)[0][-1]] = 0           # (the last stream that gets this far)
            self.ih_delta += b.dot("ih_delta", xl.T, hh)
            if self.tracked:
                self.ih_abs += np.abs(xl.T) @ np.abs(hh)
            hc = h[:, :H].copy()
            if self.mutation == "last_column_left_out" and step == 1:
                for j in np.nonzero(running & hc.any(axis=1))[0]:
                    hc[j, np.nonzero(hc[j])[0][-1]] = 0       # (the last column that carries an error)
            i_err = b.dot("chain", hc, self.ih_w.T) * live
            sq = (i_err * i_err).sum(axis=1)
            b.total("error sum", i_err, i_err, sq * running)
            # write back: h (with its cleared entries) and i_error, for the streams that run this step
            r = running[:, None]
            new_a = np.where(a_is_h[:, None], h, i_err)
            new_b = np.where(a_is_h[:, None], i_err, h)
            self.err_a, self.err_b = np.where(r, new_a, self.err_a), np.where(r, new_b, self.err_b)
            err_sum = np.where(running, sq, err_sum)
            for s in np.nonzero(running)[0]:
                self.margins.append((int(s), step, float(sq[s]), float(ceiling[s]), float(low[s]), float(max_sum[s])))
            self.ran[:, step] = running
            a_is_h = np.where(running, ~a_is_h, a_is_h)
            sq32 = sq.astype(np.float32)
            stop = (sq32 <= low) | (sq32 > max_sum)
            if self.mutation == "zero_row_runs_deeper" and step == 0:
                stop &= sq32 != 0
            t_left = np.where(running, D - step, t_left)             # (t at a break)
            running = running & ~stop
            t_left = np.where(running, D - step - 1, t_left)         # (t after the step's t--)
            offset = np.where(offset > 0, offset - 1, D - 1)
            if not running.any():
                break
        b.total("ih_delta", self.hist.reshape(-1, I), self.err_a[:, :H], self.ih_abs)
        assert (err_sum[on].astype(np.float32) <= ceiling[on]).all(), "ih_scale != 1 is not part of the construction"
        self.finals += [(int(s), float(err_sum[s]), float(ceiling[s])) for s in streams]
        self.ih_scale[on] = 1
        # the adaptive threshold (every set here has RNN_NET_FLAG_BPTT_ADAPTIVE_MIN_ERROR): a double's product, rounded once
        de = D // 4 - t_left
        move = on & (self.mef < F(1e-2)) & ((gain != low) | (de < 0))
        stepped = (self.mef.astype(np.float64) * (1.0 + de * 1e-3)).astype(np.float32)
        self.mef = np.where(move, stepped, self.mef)
        self.mef = np.where(on, np.maximum(self.mef, F(1e-20)), self.mef)
        self.depth[on] = (D - t_left)[on]
        self.generation[on] += 1
        if fused:
            self._update(self.ih_w, self.ih_delta, self.ih_m, LEARN_RATE, WEIGHTED)

    def clear_deltas(self):
        self.ho_delta[:], self.ho_abs[:], self.ih_delta[:], self.ih_abs[:] = 0, 0, 0, 0

    # -- the update --
    def apply_learning(self):
        rate = LEARN_RATE * self.c["ho_scale"]
        self._update(self.ho_w, self.ho_delta, self.ho_m, rate, self.c["method"])
        self._update(self.ih_w, self.ih_delta, self.ih_m, LEARN_RATE, self.c["method"])

    def _update(self, w, d, m, rate, method, momentum=MOMENTUM):
        """the momentum rules of rnn_apply_learning on one layer: every term a dyadic number, every sum of them exact"""
        mw = 1.0 if method == CLASSICAL else MOMENTUM_WEIGHT
        t = d * rate
        if method == NESTEROV:
            m[:] = (m + t) * momentum
            new = w + t + m
            terms = np.abs(w) + np.abs(t) + np.abs(m)
        else:
            new = w + (t + m * mw)
            terms = np.abs(w) + np.abs(t) + np.abs(m * mw)
            m[:] = (m + t) * momentum
        if self.tracked:
            k = max(99 if g is None else g for g in (Budget.grid(new), Budget.grid(m)))
            self.budget.bits["update"] = max(self.budget.bits.get("update", 0.0), float(np.log2(terms.max()) + k))
        w[:] = new

    # -- the losses of the zero-answer cases --
    def softmax_error(self, targets, n):
        """o_error = onehot - softmax of outputs that are all exactly 0: 1/n each"""
        assert not self.output.any() and n & (n - 1) == 0
        self.o_error[:] = 0
        self.o_error[:, :n] = -1.0 / n
        self.o_error[np.arange(self.S), targets] += 1.0

    def snapshot(self):
        f = np.float32
        return dict(ih_w=f(self.ih_w), ho_w=f(self.ho_w), ih_m=f(self.ih_m), ho_m=f(self.ho_m), ih_delta=f(self.ih_delta),
                    ho_delta=f(self.ho_delta), hist=f(self.hist), hidden=f(self.hidden), output=f(self.output),
                    o_error=f(self.o_error), err_a=f(self.err_a), err_b=f(self.err_b), index=self.index.copy(),
                    min_error_factor=self.mef.copy(), ih_scale=self.ih_scale.copy(), bptt_depth=self.depth.copy(),
                    generation=self.generation.copy(), top_error_raw=f(self.top_raw), top_error_scaled=f(self.top_scaled))


FLOAT_KEYS = ("hidden", "output", "hist", "o_error", "err_a", "ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "ih_scale",
              "min_error_factor")
INT_KEYS = ("bptt_depth", "index", "generation")


def first_difference(got, want, keys=FLOAT_KEYS + INT_KEYS):
    """None if every element of every array is equal (a zero's sign is not held: products with 0 may be -0), else a line
    naming the first array and element that differ and by how many units in the last place"""
    for k in keys:
        if k not in got or k not in want:
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape == b.shape and np.array_equal(a, b):
            continue
        if a.shape != b.shape:
            return "%s: shape %s against %s" % (k, a.shape, b.shape)
        bad = np.argwhere(a != b)
        i = tuple(bad[0])
        u = ""
        if a.dtype.kind == "f":
            u = ", %d ulps" % ulps(a[i], b[i])
        return "%s: %d of %d elements differ, the first at %s: %r against %r%s" % (k, len(bad), a.size, i, a[i], b[i], u)
    return None


def differences(got, want, keys=FLOAT_KEYS + INT_KEYS):
    """first_difference for every array that differs, not the first alone"""
    return [d for d in (first_difference(got, want, (k,)) for k in keys) if d is not None]


def rounded_output_bound(r):
    """per element, what a float32 sum of the output layer's H products may differ from the exact sum by, in any order,
    with or without fused multiply-adds: gamma_H sum |h w|, gamma_n = n u / (1 - n u), u = 2^-24 (the operands are exact)"""
    nu = r.H * 2.0 ** -24
    return nu / (1 - nu) * (np.abs(r.hidden) @ np.abs(r.ho_w))


def ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(key(a) - key(b)).max())


# ----------------------------------------------------------------------------- driving a case through --
# One protocol for the restatement, the oracle and the device: `steps(c)` names what happens, a driver carries it out.

def steps(c):
    """[(what, argument)]: "delta" g -- one delta generation, accumulate = accumulates(c, g); "update"; "forward" g"""
    if c["kind"] == "dyadic":
        n = generations(c)
        return [("delta", g) for g in range(n)] + [("update", None), ("forward", n)]
    return [("forward", g) for g in range(c["D"])] + [("step", c["D"]), ("forward", c["D"] + 1)]


def restated_run(c, mutation=None, budget=None, upto=None):
    """the case on the restatement: -> (the Restated, [snapshot after each compared step])"""
    net = net_of(c)
    r = Restated(c, net, mutation, budget)
    snaps = []
    text = text_of(c) if c["kind"] in ("text", "fused") else None
    after = False
    for what, g in steps(c)[:upto]:
        if what == "delta":
            r.advance()
            r.opinion(inputs_of(c, g))
            r.o_error = error_rows(c, g, net["zero_cols"]).astype(np.float64)
            r.calc_deltas(accumulates(c, g), c["ranges"], active_mask(c, g) if c["masked"] else None)
        elif what == "update":
            if c["kind"] != "fused":
                r.apply_learning()
            after = True
        elif what == "forward":
            r.advance()
            x = text_taps(text, g, c["S"])[0] if text is not None else inputs_of(c, g)
            r.opinion(x, "hidden after" if after else "hidden")
        elif what == "step":
            r.advance()
            if c["kind"] in ("text", "fused"):
                hot, tgt = text_taps(text, g, c["S"])
                r.opinion(hot)
                r.softmax_error(tgt, c["output_size"])
                r.calc_deltas(0, fused=c["kind"] == "fused")
            elif c["kind"] == "heads":
                r.opinion(head_inputs(c, g)[0])
                assert not r.output.any()
                e, cols = head_errors(c, g)
                r.o_error[:] = e
                r.calc_deltas(0, stream_cols=cols)
            else:
                r.opinion(inputs_of(c, g))
                assert not r.output.any()
                r.clear_deltas()
                r.o_error[:] = 0
                if c["kind"] == "sigmoid":      # the answers become their sigmoid in place: exactly 1/2
                    n = c["output_size"]
                    r.output[:, :n] = 0.5
                    r.o_error[:, :n] = 0.25 * (sigmoid_targets(c, g).astype(np.float64) - 0.5)
                    r.calc_deltas(1)
                else:
                    e, trained = group_errors(c, g)[:2]
                    r.o_error[:] = e
                    r.calc_deltas(1, None, trained)
            if c["kind"] != "fused":
                r.apply_learning()
            after = True
        snaps.append(r.snapshot())
    return r, snaps


class OracleSide:
    """the case on oracle/liboracle.so (float32, in the reference's own order of summation)"""

    def __init__(self, c, net=None):
        import recur_ctypes as rc
        import scenarios as sc
        self.rc, self.c = rc, c
        self.net = net = net or net_of(c)
        self.o = o = sc.OracleSet(input_size=c["input_size"], hidden_size=c["hidden_size"], output_size=c["output_size"],
                                  S=c["S"], D=c["D"], activation=c["activation"], learn_rate=LEARN_RATE, seed=c["seed"])
        a = o.arrays()
        for k in ("ih_w", "ho_w", "ih_m", "ho_m"):
            assert a[k].shape == net[k].shape
            a[k][:] = net[k]
        a["ih_aux"][:] = 0
        a["ho_aux"][:] = 0
        o.z.contents.ho_scale = c["ho_scale"]
        o.z.contents.momentum_weight = MOMENTUM_WEIGHT
        self.text = text_of(c) if c["kind"] in ("text", "fused") else None
        self.ranges = None if not c["ranges"] else np.array(range_pairs(c), np.int32)

    def _opinion(self, j, x):
        if np.ndim(x) == 1:
            self.o.orc.orc_one_hot_opinion(self.o.z, j, int(x[j]), 0.0)
        else:
            self.o.orc.orc_opinion(self.o.z, j, self.rc.fptr(np.ascontiguousarray(x[j], np.float32)), 0.0)

    def delta(self, g):
        c, o = self.c, self.o
        x, e, act = inputs_of(c, g), error_rows(c, g, self.net["zero_cols"]), active_mask(c, g)
        a = o.arrays()
        for j in range(c["S"]):
            o.orc.orc_advance(o.z, j)
            self._opinion(j, fed(c, x))
            a["o_error"][j] = e[j]
            if act[j]:
                o.orc.orc_calc_deltas(o.z, j, 1 if (j or accumulates(c, g)) else 0, None if self.ranges is None else self.rc.iptr(self.ranges))

    def update(self):
        self.o.orc.orc_apply_learning(self.o.z, self.c["method"], MOMENTUM)

    def forward(self, g):
        x = text_taps(self.text, g, self.c["S"])[0] if self.text is not None else fed(self.c, inputs_of(self.c, g))
        for j in range(self.c["S"]):
            self.o.orc.orc_advance(self.o.z, j)
            self._opinion(j, x)

    def step(self, g):
        c, o, rc = self.c, self.o, self.rc
        if c["kind"] == "text":
            o.char_step(self.text, g, c["method"], MOMENTUM)
            return
        import ctypes as C
        if c["kind"] == "fused":
            hit = C.c_int(0)
            o.orc.orc_advance(o.z, 0)
            o.orc.orc_net_error_bptt(o.z, 0, int(self.text[g]), int(self.text[g + 1]), C.byref(hit))
            o.orc.orc_bptt_calculate(o.z, 0, 1, MOMENTUM)
            return
        if c["kind"] == "heads":
            hot, nxt, cls = head_inputs(c, g)
            heads = c["output_size"] // c["input_size"]
            ranges = (C.c_int * (2 * (heads + 1)))()
            self.own_error = []
            for j in range(c["S"]):
                o.orc.orc_advance(o.z, j)
                self.own_error.append(o.orc.orc_multi_softmax_error(o.z, j, int(hot[j]), int(nxt[j]), int(cls[j]),
                                                                    c["input_size"], c["leakage"], ranges))
                o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, ranges)
            o.orc.orc_apply_learning(o.z, c["method"], MOMENTUM)
            return
        x = inputs_of(c, g)
        o.orc.orc_clear_deltas(o.z)
        if c["kind"] == "groups":
            goff, gsize = group_layout()
            t, w = group_targets(c, g), group_weights(c)
            self.wins, self.wrong, self.groups = C.c_int(0), C.c_float(0), 0
        for j in range(c["S"]):
            o.orc.orc_advance(o.z, j)
            self._opinion(j, x)
            if c["kind"] == "sigmoid":
                o.orc.orc_sigmoid_mse_error(o.z, j, rc.fptr(np.ascontiguousarray(sigmoid_targets(c, g)[j])), c["output_size"])
                o.orc.orc_calc_deltas(o.z, j, 1, None)
            else:
                k = o.orc.orc_grouped_softmax_error(o.z, j, len(gsize), rc.iptr(goff), rc.iptr(gsize),
                                                    rc.iptr(np.ascontiguousarray(t[j])), rc.fptr(w), C.byref(self.wins),
                                                    C.byref(self.wrong))
                self.groups += k
                if k:
                    o.orc.orc_calc_deltas(o.z, j, 1, None)
        o.orc.orc_apply_learning(o.z, c["method"], MOMENTUM)

    def run(self, what, g):
        getattr(self, what)(*(() if what == "update" else (g,)))

    def snapshot(self):
        return self.o.snapshot()

    def close(self):
        self.o.close()


def oracle_run(c):
    """the case on the oracle: -> [snapshot after each compared step]"""
    side = OracleSide(c)
    snaps = []
    for what, g in steps(c):
        side.run(what, g)
        snaps.append(side.snapshot())
    side.close()
    return snaps


def budget(c):
    """the bits every sum of the case uses, by stage: -> (dict stage -> bits, the stages over the limit)"""
    b = Budget()
    restated_run(c, budget=b)
    return b.bits, b.over()
