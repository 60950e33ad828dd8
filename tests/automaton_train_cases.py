"""What tests/test_automaton_train_rule.py, tests/test_automaton_train_cases_cpu.py and tests/test_gpu_automaton_training.py
share: the numpy float32 restatement of recur_amd/csrc/automaton_train_rule.h (gstrnnca.c: fill_net_inputs 669-691, the
targets of train_net 702-708, the momentum of maybe_learn 726-728), its broken forms, the grids and films of the cases, the
loop of separate calls the block call is held to, and the oracle twin of a generation of rnnca's trainer.  numpy rounds
every float32 operation once and fuses none, which is the rule."""
import numpy as np

import recur_ctypes as rc
import scenarios as sc
from test_automaton_rule import DEFAULT_C, DEFAULT_Y

F = np.float32
BROKEN = ("x and y swapped", "Cb and Cr swapped in the inputs", "Cb and Cr swapped in the targets",
          "the target from frame t", "the target's plane stride", "divide by 255", "wrap for clamp")
MOMENTUM = 0.5           # gstrnnca.c: DEFAULT_PROP_MOMENTUM


class Grid:
    """a grid and what a cell sees of it: AutomatonRule's fields, the offset lists as [(dx, dy)]"""

    def __init__(self, width, height, ys=DEFAULT_Y, cs=DEFAULT_C, len_pos=2, edges=1):
        self.width, self.height, self.ys, self.cs, self.len_pos, self.edges = width, height, list(ys), list(cs), len_pos, edges
        self.input_size = len(self.ys) + 2 * len(self.cs) + len_pos

    def geometry(self):
        from recur_amd.drivers import AutomatonGeometry
        return AutomatonGeometry(self.width, self.height, np.array(self.ys, np.int32).reshape(-1, 2),
                                 np.array(self.cs, np.int32).reshape(-1, 2), self.len_pos, self.edges)


def np_unit(b, broken=None):
    """BYTE_TO_UNIT: the byte times the rounded reciprocal of 255 -- not the quotient"""
    b = np.asarray(b).astype(F)
    if broken == "divide by 255":
        return (b / F(255.0)).astype(F)
    return (b * (F(1.0) / F(255.0))).astype(F)


def unit_differs():
    """the bytes whose product with the rounded reciprocal is not their quotient by 255"""
    b = np.arange(256)
    return b[np_unit(b) != np_unit(b, "divide by 255")]


def np_source(g, dx, dy, x, y, broken=None):
    """gstrnnca.c:644-667 for arrays of cells: the source cell of offset (dx, dy)"""
    w, h = g.width, g.height
    sx, sy = x + dx, y + dy
    clamp = bool(g.edges)
    if broken == "wrap for clamp":
        clamp = not clamp
    if clamp:
        sy = np.clip(sy, 0, h - 1)
        sx = np.clip(sx, 0, w - 1)
    else:
        sy = np.where(sy < 0, sy + h, np.where(sy >= h, sy - h, sy))
        sx = np.where(sx < 0, sx + w, np.where(sx >= w, sx - w, sx))
    return sy * w + sx


def np_positions(g, x, y):
    """the position inputs [n][len_pos] (gstrnnca.c:684-690): the third in double, rounded once"""
    xx = ((x.astype(F) * F(1.0)) / F(g.width)).astype(F)
    yy = ((y.astype(F) * F(1.0)) / F(g.height)).astype(F)
    cols = [xx, yy]
    if g.len_pos == 3:
        x64, y64 = xx.astype(np.float64), yy.astype(np.float64)
        cols.append((0.5 - ((y64 - 0.5) * (y64 - 0.5) + (x64 - 0.5) * (x64 - 0.5))).astype(F))
    return np.stack(cols, axis=1)


def per_step(xy, T):
    """xy [n][2] or [T][n][2] -> [T][n][2]"""
    xy = np.asarray(xy, np.int32)
    return np.broadcast_to(xy, (T,) + xy.shape).copy() if xy.ndim == 2 else xy


def np_block(g, frames, xy, broken=None):
    """-> (rows float32 [T][n][input_size], targets float32 [T][n][3]) of a film uint8 [T + 1][3][height][width] and the
    trainers' (x, y), [n][2] or [T][n][2]"""
    frames = np.asarray(frames, np.uint8)
    T = frames.shape[0] - 1
    cells = g.width * g.height
    flat = frames.reshape(-1)
    planes = frames.reshape(T + 1, 3, cells)
    pos = per_step(xy, T)
    rows = np.zeros((T, pos.shape[1], g.input_size), F)
    targets = np.zeros((T, pos.shape[1], 3), F)
    for t in range(T):
        x, y = pos[t, :, 0].astype(np.int64), pos[t, :, 1].astype(np.int64)
        if broken == "x and y swapped":
            x, y = np.minimum(y, g.width - 1), np.minimum(x, g.height - 1)   # (kept on the grid where it is not square)
        cols = [np_unit(planes[t, 0, np_source(g, dx, dy, x, y, broken)], broken) for dx, dy in g.ys]
        for dx, dy in g.cs:
            at = np_source(g, dx, dy, x, y, broken)
            pair = [np_unit(planes[t, 1, at], broken), np_unit(planes[t, 2, at], broken)]
            cols += pair[::-1] if broken == "Cb and Cr swapped in the inputs" else pair
        rows[t] = np.concatenate([np.stack(cols, axis=1).reshape(len(x), -1), np_positions(g, x, y)], axis=1)
        own = y * g.width + x
        for k in range(3):
            plane = {1: 2, 2: 1}.get(k, k) if broken == "Cb and Cr swapped in the targets" else k
            frame = t if broken == "the target from frame t" else t + 1
            stride = g.width if broken == "the target's plane stride" else cells
            targets[t, :, k] = np_unit(flat[frame * 3 * cells + plane * stride + own], broken)
    return rows, targets


def np_momenta(generation0, T, momentum, soft_start):
    """the momentum of T generations from net generation generation0 (rnn_calculate_momentum_soft_start in float32)"""
    if soft_start == 0:
        return [F(momentum)] * T
    x = F(soft_start)
    return [min(F(momentum), F(F(1.0) - x / (F(F(1.0) + F(generation0 + t)) + F(F(2.0) * x)))) for t in range(T)]


# ------------------------------------------------------------------ films and positions --

PLANTED = np.array([0, 1, 254, 255], np.uint8)


def film_of(g, T, seed):
    """random bytes [T + 1][3][height][width]"""
    return np.random.default_rng(seed).integers(0, 256, (T + 1, 3, g.height, g.width), dtype=np.uint8)


def plant(g, film, xy):
    """0, 1, 254 and 255 under the trainers and their neighbours, in every frame and plane (in place)"""
    pos = per_step(xy, film.shape[0] - 1)
    for t in range(film.shape[0]):
        p = pos[min(t, len(pos) - 1)]
        for j, (x, y) in enumerate(p):
            for k, (dx, dy) in enumerate([(0, 0), (1, 0), (0, 1), (-1, -1)]):
                for plane in range(3):
                    film[t, plane, (y + dy) % g.height, (x + dx) % g.width] = PLANTED[(j + k + plane + t) % 4]
    return film


def every_cell(g):
    """a trainer on every cell, (x, y) pairs in cell order"""
    return np.array([(x, y) for y in range(g.height) for x in range(g.width)], np.int32)


def random_xy(g, n, seed, T=None):
    """n trainers' (x, y) anywhere on the grid (cells may repeat), [n][2] or with T [T][n][2], one moved every step"""
    rs = np.random.default_rng(seed)
    xy = np.stack([rs.integers(0, g.width, n), rs.integers(0, g.height, n)], axis=1).astype(np.int32)
    if T is None:
        return xy
    out = np.zeros((T, n, 2), np.int32)
    for t in range(T):
        out[t] = xy
        xy = xy.copy()
        xy[rs.integers(0, n)] = (rs.integers(0, g.width), rs.integers(0, g.height))
    return out


RULE_GRIDS = [Grid(3, 3), Grid(5, 4), Grid(16, 12)]


def rule_cases():
    """(name, grid, T, xy) of the rule test: every grid clamped and wrapped, len_pos 2 and 3, an empty C list"""
    out = []
    for base in RULE_GRIDS:
        for edges in (1, 0):
            for len_pos in (2, 3):
                g = Grid(base.width, base.height, len_pos=len_pos, edges=edges)
                xy = every_cell(g) if g.width == 3 else random_xy(g, 7, [g.width, edges, len_pos], T=3)
                out.append(("%dx%d edges %d pos %d" % (g.width, g.height, edges, len_pos), g, 3, xy))
    g = Grid(5, 4, cs=[], len_pos=3)
    out.append(("5x4 no C", g, 2, random_xy(g, 4, 5)))
    return out


def pattern_of(g):
    """an offset pattern that parses into g's lists: the default, or the default's Y list alone"""
    assert g.ys == DEFAULT_Y and g.cs in (DEFAULT_C, [])
    return "Y00120111C0111" if g.cs else "Y00120111"


# ------------------------------------------------------------------ the loop the block call is held to --

def run_loop(lib, gs, g, film, xy, advance=False, momenta=None, momentum=MOMENTUM, condition=False, style=rc.WEIGHTED):
    """today's loop on an AmdBatchedSet: per generation the rows gathered by the restatement, rnn_amd_set_advance where
    `advance`, rnn_amd_set_dense_step_sigmoid_mse, rnn_condition_net where `condition`.  -> the float64 sum of the terms
    (target - a)^2 cannot be had from this loop: the statistics are the block call's alone"""
    rows, targets = np_block(g, film, xy)
    for t in range(rows.shape[0]):
        x, tg = np.ascontiguousarray(rows[t]), np.ascontiguousarray(targets[t])
        if advance:
            lib.rnn_amd_set_advance(gs.handle)
        m = momentum if momenta is None else float(momenta[t])
        lib.rnn_amd_set_dense_step_sigmoid_mse(gs.handle, rc.fptr(x), x.shape[1], rc.fptr(tg), 3, 3, style, m)
        if condition:
            lib.rnn_condition_net(gs.net)


# ------------------------------------------------------------------ the oracle twin --

def oracle_generation(o, x, t, momentum, advance, update=True):
    """one generation of rnnca's trainer on an OracleSet: orc_clear_deltas; per trainer orc_advance where `advance`,
    orc_opinion, orc_sigmoid_mse_error on three outputs, orc_calc_deltas summed; orc_apply_learning.
    -> the loss terms (target - a)^2, float32 [S][3]"""
    orc, z = o.orc, o.z
    a = o.arrays()
    orc.orc_clear_deltas(z)
    terms = np.zeros((o.S, 3), F)
    for j in range(o.S):
        if advance:
            orc.orc_advance(z, j)
        orc.orc_opinion(z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
        orc.orc_sigmoid_mse_error(z, j, rc.fptr(np.ascontiguousarray(t[j])), 3)
        d = (np.asarray(t[j], F) - a["output"][j, :3]).astype(F)
        terms[j] = (d * d).astype(F)
        orc.orc_calc_deltas(z, j, 1, None)
    if update:
        orc.orc_apply_learning(z, rc.WEIGHTED, momentum)
    return terms


def oracle_block(o, g, film, xy, advance=False, momentum=MOMENTUM, soft_start=0.0):
    """the block on the oracle alone -> the mean squared error of each generation"""
    rows, targets = np_block(g, film, xy)
    gen0 = int(o.arrays()["generation"][0])
    momenta = np_momenta(gen0, rows.shape[0], momentum, soft_start)
    return [float(oracle_generation(o, rows[t], targets[t], float(momenta[t]), advance).astype(np.float64).mean())
            for t in range(rows.shape[0])]


# ------------------------------------------------------------------ the cases that must be able to notice --

SENS = dict(grid=Grid(5, 4), hidden=24, n=6, D=4, T=5, seed=41, learn_rate=1e-2)
PARITY_BAR = 1e-4        # the project's parity bar (tests/test_gpu_callers.py: RTOL)


def sens_kw(c=SENS):
    return dict(input_size=c["grid"].input_size, hidden_size=c["hidden"], output_size=3, S=c["n"], D=c["D"],
                learn_rate=c["learn_rate"], seed=c["seed"], momentum=MOMENTUM)


def sens_data(c=SENS):
    g = c["grid"]
    xy = random_xy(g, c["n"], 3, T=c["T"])
    return plant(g, film_of(g, c["T"], 17), xy), xy


# ------------------------------------------------------------------ the learning case --
# A film whose every frame is the one before moved one pixel to the right, wrapped: the pixel at (x, y) of frame t + 1 is
# the pixel at (x - 1, y) of frame t, in every plane.  The offset list "Y01C01" holds (-1, 0) for both, so one neighbour
# offset per plane expresses the rule.  The picture is smooth (a sum of two sines per plane) so that the levels vary.

LEARN = dict(width=16, height=12, pattern="Y01C01", trainers=40, hidden=16, depth=4, rate=0.01, momentum=0.5, generations=640,
             block=64, seed=11)
LEARN_FACTOR = 0.5       # the tool's last block must be below this share of its first: the CPU half shows it for the oracle


def learning_film(generations=None):
    """-> uint8 [generations + 1][3][height][width]"""
    L = LEARN
    T = (L["generations"] if generations is None else generations) + 1
    x, y = np.meshgrid(np.arange(L["width"]), np.arange(L["height"]))
    film = np.zeros((T, 3, L["height"], L["width"]), np.uint8)
    for plane in range(3):
        base = 128 + 70 * np.sin(2 * np.pi * (x * (plane + 1)) / L["width"]) + 40 * np.cos(2 * np.pi * y / L["height"] + plane)
        for t in range(T):
            film[t, plane] = np.roll(np.clip(base, 0, 255).astype(np.uint8), t, axis=1)
    return film


def learning_grid():
    ys = [(0, 1), (0, -1), (1, 0), (-1, 0)]      # what setup_inputs makes of "01"
    return Grid(LEARN["width"], LEARN["height"], ys=ys, cs=ys, len_pos=2, edges=1)
