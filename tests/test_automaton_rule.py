"""How rnnca's automaton makes the next frame, asked of the rule itself (recur_amd/csrc/automaton_rule.h, what
k_automaton_step runs on the device) without a GPU: automaton_rule_harness.cpp is compiled with g++ alone, takes the
oracle's exponential (liboracle.so) as the level rule's functor and prints source cells, input rows, levels and offset
lists.  The expected values are a numpy restatement of gstrnnca.c:375-439 and 644-691 in float32 / float64 arithmetic and
orc_fast_sigmoid with a truncation, and must be met bit for bit.  The restatement is then broken one rule at a time, and
each broken form must differ on the small grids the device tests use: they would notice that rule being wrong.  And the
refusals of rnn_amd_run_automaton, which come before anything needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "automaton_rule_harness.cpp")
ORACLE_DIR = os.path.join(ROOT, "oracle")
CXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
LINK = ["-L", ORACLE_DIR, "-l:liboracle.so", "-Wl,-rpath," + ORACLE_DIR]
DEFAULT = "Y00120111C0111"
# what setup_inputs makes of the default pattern, written out by hand: "00", "12", "01", "11" for Y, "01", "11" for C --
# per digit pair (min, max): y and -y, then the same for -x, then the same again with x and y swapped
DEFAULT_Y = [(0, 0),
             (1, 2), (1, -2), (-1, 2), (-1, -2), (2, 1), (2, -1), (-2, 1), (-2, -1),
             (0, 1), (0, -1), (1, 0), (-1, 0),
             (1, 1), (1, -1), (-1, 1), (-1, -1)]
DEFAULT_C = [(0, 1), (0, -1), (1, 0), (-1, 0),
             (1, 1), (1, -1), (-1, 1), (-1, -1)]
GRIDS = [(5, 4), (3, 3)]
F = np.float32


@pytest.fixture(scope="module")
def orc():
    return rc.load_oracle()  # (builds oracle/liboracle.so where it is missing)


def build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "automaton_rule_harness")
    subprocess.run(CXX + list(extra) + [SRC, "-o", exe] + LINK, check=True)
    return exe


@pytest.fixture(scope="module")
def harness(orc, tmp_path_factory):
    return build(tmp_path_factory, "automaton_rule")


@pytest.fixture(scope="module")
def sanitized(orc, tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: it has its own main, so the runtimes are
    linked into it and nothing is preloaded"""
    return build(tmp_path_factory, "automaton_rule_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def ask(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def numbers(exe, *args):
    return np.array(ask(exe, *args).split(), np.int64)


def test_the_header_needs_no_hip_and_is_c_as_well():
    hdr = os.path.join(CSRC, "automaton_rule.h")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c++",
                    hdr], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c", hdr],
                   check=True)


# ------------------------------------------------------------------ the source cell --

def reaches(dx, dy, w, h):
    return abs(dx) < w and abs(dy) < h


def source(dx, dy, cx, cy, w, h, edges, broken=None):
    """gstrnnca.c:644-667, and its broken forms"""
    x, y = cx + dx, cy + dy
    if broken == "x and y swapped":
        x, y = cx + dy, cy + dx
    clamp = bool(edges)
    if broken == "clamp for wrap":
        clamp = not clamp
    if clamp:
        y = max(0, min(h - 1, y))
        x = max(0, min(w - 1, x))
    elif broken == "wrap twice":
        x, y = x % w, y % h   # (as often as it takes)
    else:
        if y < 0:
            y += h
        elif y >= h:
            y -= h
        if x < 0:
            x += w
        elif x >= w:
            x -= w
    return y * (h if broken == "y * height" else w) + x


def all_sources(w, h, edges, reach=3, broken=None, raw=False):
    """raw: every offset is asked, also those the single wrap does not bring back (the call refuses them)"""
    out = []
    for cy in range(h):
        for cx in range(w):
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    ok = raw or edges or reaches(dx, dy, w, h)
                    out.append(source(dx, dy, cx, cy, w, h, edges, broken) if ok else -1)
    return np.array(out, np.int64)


def check_sources(exe):
    for w, h in GRIDS:
        for edges in (1, 0):
            got = numbers(exe, "source", w, h, edges, 3)
            want = all_sources(w, h, edges)
            assert np.array_equal(got, want), (w, h, edges)
            asked = got[got >= 0]
            assert asked.max() == w * h - 1 and asked.min() == 0 and len(asked) >= w * h * (9 if not edges else 49)
    # in wrap mode only the offsets the call accepts are asked: on 3 x 3 that is [-2, 2]^2
    assert (numbers(exe, "source", 3, 3, 0, 3) >= 0).sum() == 9 * 25


def test_source_cells_are_the_references(harness):
    check_sources(harness)


@pytest.mark.parametrize("broken", ["clamp for wrap", "x and y swapped", "y * height"])
def test_each_source_rule_is_noticed(harness, broken):
    differ = 0
    for w, h in GRIDS:
        for edges in (1, 0):
            differ += not np.array_equal(numbers(harness, "source", w, h, edges, 3), all_sources(w, h, edges, broken=broken))
    assert differ >= 1, broken
    if broken == "y * height":   # (a square grid cannot see it: the 5 x 4 one must)
        assert not np.array_equal(numbers(harness, "source", 5, 4, 1, 3), all_sources(5, 4, 1, broken=broken))


def test_the_wrap_is_a_single_one(harness):
    """Wherever the single wrap reaches it IS the full one, so no offset the call accepts can tell them apart: the rule is
    asked raw, beyond what the call accepts (reach 4 on 3 x 3).  There it does what the reference does -- one width or
    height, and the cell lies outside the plane, which is why the call refuses such offsets -- and the full wrap differs."""
    got = numbers(harness, "rawsource", 3, 3, 0, 4)
    assert np.array_equal(got, all_sources(3, 3, 0, reach=4, raw=True))
    assert not np.array_equal(got, all_sources(3, 3, 0, reach=4, raw=True, broken="wrap twice"))
    assert got.max() > 8 or got.min() < 0
    inside = all_sources(3, 3, 0, reach=4) >= 0
    assert np.array_equal(got[inside], all_sources(3, 3, 0, reach=4, raw=True, broken="wrap twice")[inside])


# ------------------------------------------------------------------ the input row --

def input_rows(frame, w, h, edges, len_pos, ys, cs, broken=None):
    """gstrnnca.c:669-691 in numpy float32 / float64 arithmetic: [cells][len_y + 2 * len_c + len_pos] float32"""
    planes = frame.reshape(3, w * h)
    recip = F(1.0) / F(255.0)

    def unit(b):
        return F(b) / F(255.0) if broken == "divide by 255" else F(b) * recip

    rows = []
    for cy in range(h):
        for cx in range(w):
            row = [unit(planes[0, source(dx, dy, cx, cy, w, h, edges)]) for dx, dy in ys]
            for dx, dy in cs:
                at = source(dx, dy, cx, cy, w, h, edges)
                pair = [unit(planes[1, at]), unit(planes[2, at])]
                row += pair[::-1] if broken == "Cb and Cr swapped" else pair
            xx = F(cx) * F(1.0) / F(w)
            yy = F(cy) * F(1.0) / F(h)
            row += [xx, yy]
            if len_pos == 3:
                if broken == "third position in float":
                    row.append(F(0.5) - ((yy - F(0.5)) * (yy - F(0.5)) + (xx - F(0.5)) * (xx - F(0.5))))
                else:
                    x64, y64 = np.float64(xx), np.float64(yy)
                    row.append(F(0.5 - ((y64 - 0.5) * (y64 - 0.5) + (x64 - 0.5) * (x64 - 0.5))))
            rows.append(np.array(row, F))
    return np.stack(rows)


def frame_of(w, h, seed):
    f = np.random.default_rng(seed).integers(0, 256, 3 * w * h, dtype=np.uint8)
    f[:4] = [0, 255, 1, 254]
    return f


def harness_rows(exe, tmp_path, frame, w, h, edges, len_pos, pattern=DEFAULT):
    path = str(tmp_path / ("frame_%d_%d.u8" % (w, h)))
    frame.tofile(path)
    bits = numbers(exe, "inputs", w, h, edges, len_pos, pattern, path).astype(np.uint32)
    return bits.reshape(w * h, -1)


def check_inputs(exe, tmp_path):
    for w, h in GRIDS + [(7, 3)]:
        frame = frame_of(w, h, 10 * w + h)
        for edges in (1, 0):
            for len_pos in (2, 3):
                got = harness_rows(exe, tmp_path, frame, w, h, edges, len_pos)
                want = input_rows(frame, w, h, edges, len_pos, DEFAULT_Y, DEFAULT_C)
                assert got.shape == (w * h, 17 + 16 + len_pos)
                assert np.array_equal(got, want.view(np.uint32)), (w, h, edges, len_pos)


def test_input_rows_are_the_references_bit_for_bit(harness, tmp_path):
    check_inputs(harness, tmp_path)


@pytest.mark.parametrize("broken", ["divide by 255", "third position in float", "Cb and Cr swapped"])
def test_each_input_rule_is_noticed(harness, tmp_path, broken):
    differ = 0
    for w, h in GRIDS + [(7, 3)]:
        frame = frame_of(w, h, 10 * w + h)
        got = harness_rows(harness, tmp_path, frame, w, h, 1, 3)
        differ += not np.array_equal(got, input_rows(frame, w, h, 1, 3, DEFAULT_Y, DEFAULT_C, broken).view(np.uint32))
    assert differ >= 1, broken


def test_the_reciprocal_and_the_division_differ_on_some_byte():
    """(why the rule says which: 1.0f / 255.0f is rounded, and its product is not every byte's quotient)"""
    b = np.arange(256, dtype=F)
    assert np.any(b * (F(1.0) / F(255.0)) != b / F(255.0))


# ------------------------------------------------------------------ the level --

def level_inputs():
    g = np.random.default_rng(8)
    x = np.concatenate([np.linspace(-12.0, 12.0, 4001), g.uniform(-1e4, 1e4, 300), g.standard_normal(300) * 3.0,
                        [0.0, -0.0, 50.0, -50.0, 87.0, -87.0, 100.0, -100.0, 1e3, -1e3, 1e4, -1e4]])
    return x.astype(F)


def want_level(orc, x):
    a = F(orc.orc_fast_sigmoid(float(x)))
    return int(a * F(255.9))


def check_levels(exe, orc, tmp_path):
    x = level_inputs()
    path = str(tmp_path / "outputs.f32")
    np.concatenate([x, np.array([np.nan, np.inf, -np.inf], F)]).tofile(path)
    got = numbers(exe, "level", path)
    want = np.array([want_level(orc, v) for v in x], np.int64)
    assert np.array_equal(got[:len(x)], want)
    assert want.min() == 0 and want.max() == 255 and len(np.unique(want)) == 256      # both ends and all between
    # what the oracle cannot be asked (its exponential's range reduction does not end on an infinity): NaN stores 0, the
    # infinities take the limits
    assert list(got[len(x):]) == [0, 255, 0]
    # the cases C leaves undefined, on the scaled value itself
    scaled = np.array([0.0, -0.0, 0.99, 1.0, 255.0, 255.9, 255.99, 256.0, 300.0, 1e30, np.inf, -0.5, -1.0, -1e30, -np.inf,
                       np.nan], F)
    path = str(tmp_path / "scaled.f32")
    scaled.tofile(path)
    assert list(numbers(exe, "byte", path)) == [0, 0, 0, 1, 255, 255, 255, 255, 255, 255, 255, 0, 0, 0, 0, 0]


def test_levels_are_the_oracles_sigmoid_truncated_bit_for_bit(harness, orc, tmp_path):
    check_levels(harness, orc, tmp_path)


# ------------------------------------------------------------------ the offset pattern --

def pattern(exe, string, room):
    d = dict(line.split("=", 1) for line in ask(exe, "pattern", string, room).splitlines())

    def pairs(s):
        return [tuple(int(v) for v in p.split(",")) for p in s.split(";")] if s else []

    return int(d["rc"]), pairs(d["y"]), pairs(d["c"])


def check_patterns(exe):
    assert pattern(exe, DEFAULT, 17) == (0, DEFAULT_Y, DEFAULT_C)          # room for exactly the longer list
    assert len(DEFAULT_Y) == 17 and len(DEFAULT_C) == 8 and 17 + 2 * 8 + 2 == 35
    assert pattern(exe, "Y00", 1) == (0, [(0, 0)], [])
    assert pattern(exe, "Y12", 8) == (0, DEFAULT_Y[1:9], [])
    assert pattern(exe, "Y21", 8) == (0, DEFAULT_Y[1:9], [])               # (min, max) whatever the order
    assert pattern(exe, "C11", 4) == (0, [], DEFAULT_C[4:])
    assert pattern(exe, "11", 4) == (0, DEFAULT_C[4:], [])                 # the Y list is the one to start with
    assert pattern(exe, "Y0x0 C;1?1", 4) == (0, [(0, 0)], DEFAULT_C[4:])   # unknown characters are skipped
    assert pattern(exe, "Y001", 4) == (0, [(0, 0)], [])                    # half a pair is none
    assert pattern(exe, "", 0) == (0, [], [])
    # arrays too small: refused, nothing written behind them (the sanitized build would say), the lists as far as they got
    assert pattern(exe, DEFAULT, 16) == (-1, DEFAULT_Y[:16], [])
    assert pattern(exe, DEFAULT, 7)[0] == -1 and pattern(exe, "Y12", 7) == (-1, DEFAULT_Y[1:8], [])
    assert pattern(exe, "C01", 0) == (-1, [], [])


def test_the_default_pattern_and_its_relatives(harness):
    check_patterns(harness)


def test_under_address_and_undefined_behaviour_sanitizers(sanitized, orc, tmp_path):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it"""
    check_sources(sanitized)
    check_inputs(sanitized, tmp_path)
    check_levels(sanitized, orc, tmp_path)
    check_patterns(sanitized)


# ------------------------------------------------------------------ the call's refusals need no device --

@pytest.fixture(scope="module")
def lib():
    return rc.bind_char(rc.load_amd())


def test_parse_offsets_through_the_library(lib):
    from recur_amd.drivers import parse_offsets
    ys, cs = parse_offsets(lib, DEFAULT)
    assert [tuple(p) for p in ys] == DEFAULT_Y and [tuple(p) for p in cs] == DEFAULT_C
    with pytest.raises(ValueError):
        parse_offsets(lib, DEFAULT, max_pairs=16)      # (the driver asserts that nothing lies behind the room)
    ny, nc = C.c_int(0), C.c_int(0)
    room = np.zeros(64, np.int32)
    assert lib.rnn_amd_automaton_parse_offsets(None, rc.iptr(room), C.byref(ny), rc.iptr(room), C.byref(nc), 32) == -1
    assert lib.rnn_amd_automaton_parse_offsets(b"Y00", None, C.byref(ny), rc.iptr(room), C.byref(nc), 32) == -1
    assert lib.rnn_amd_automaton_parse_offsets(b"Y00", rc.iptr(room), C.byref(ny), rc.iptr(room), C.byref(nc), -1) == -1


def test_refusals_and_the_early_return_need_no_device(lib):
    """-1 with nothing written, and 0 for no frames, on a machine without a GPU (no compute entry point is reached; with a
    device present the same calls return before they touch it)"""
    from recur_amd.drivers import AutomatonGeometry
    net = lib.rnn_new(35, 39, 3, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    net36 = lib.rnn_new(36, 39, 3, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    two = lib.rnn_new(35, 39, 2, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(20, 35, 39, 3, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    H = net.contents.h_size
    w, h = 5, 4
    seed = np.full(3 * w * h, 7, np.uint8)
    frames = np.full(2 * 3 * w * h, 0xEE, np.uint8)
    h_in = np.random.default_rng(1).random((w * h, H)).astype(np.float32)
    h_out = np.full((w * h, H), 5.0, np.float32)

    def geometry(width=w, height=h, ys=DEFAULT_Y, cs=DEFAULT_C, len_pos=2, edges=1, **over):
        g = AutomatonGeometry(width, height, ys, cs, len_pos, edges)
        for k, v in over.items():
            setattr(g.struct, k, v)
        call.keep = getattr(call, "keep", []) + [g]
        return C.byref(g.struct)

    def call(net=net, ca=None, seed=rc.u8ptr(seed), n=2, h_in=rc.fptr(h_in), h_out=rc.fptr(h_out), segment=0,
             frames=rc.u8ptr(frames)):
        return lib.rnn_amd_run_automaton(net, geometry() if ca is None else ca, seed, n, h_in, h_out, segment, frames)

    assert call(net=None) == -1 and call(seed=None) == -1 and call(frames=None) == -1
    assert lib.rnn_amd_run_automaton(net, None, rc.u8ptr(seed), 2, None, None, 0, rc.u8ptr(frames)) == -1
    assert call(n=-1) == -1
    assert call(ca=geometry(width=0)) == -1 and call(ca=geometry(height=-3)) == -1
    assert call(ca=geometry(width=1 << 16, height=1 << 15)) == -1                        # 2^31 cells
    assert call(ca=geometry(len_y=-1)) == -1 and call(ca=geometry(len_c=-1)) == -1
    assert call(ca=geometry(offsets_y=None)) == -1 and call(ca=geometry(offsets_c=None)) == -1
    assert call(ca=geometry(len_pos=1)) == -1 and call(ca=geometry(len_pos=4)) == -1
    assert call(ca=geometry(len_pos=3)) == -1 and call(net=net36) == -1                  # 36 inputs and 35, both ways
    assert call(net=net36, ca=geometry(len_pos=3), n=0, h_in=None, h_out=None) == 0      # (the two that fit)
    assert call(ca=geometry(ys=DEFAULT_Y[:16])) == -1
    assert call(net=two) == -1                                                           # two outputs are no pixel
    assert call(net=bottom) == -1                                                        # a bottom layer
    # a wrapped grid the offsets do not fit: the default reaches 2, so 2 columns or 2 rows are too few, 3 are enough
    assert call(ca=geometry(width=2, height=10, edges=0)) == -1 and call(ca=geometry(width=10, height=2, edges=0)) == -1
    assert call(ca=geometry(width=3, height=3, edges=0), n=0, h_in=None, h_out=None) == 0
    far = [(0, 0)] * 16 + [(0, -4)]
    assert call(ca=geometry(ys=far, edges=0)) == -1
    assert np.all(frames == 0xEE) and np.all(h_out == 5.0)                               # nothing written
    # no frames: 0 at once, no device asked for, the states copied by the host alone
    assert call(n=0, frames=None) == 0
    assert np.array_equal(h_out[:, 1:40], h_in[:, 1:40]) and np.all(frames == 0xEE)
    same = h_in.copy()
    assert call(n=0, h_in=rc.fptr(same), h_out=rc.fptr(same)) == 0 and np.array_equal(same[:, 1:40], h_in[:, 1:40])
    assert call(n=0, h_out=None) == 0 and call(n=0, h_in=None, h_out=None) == 0
    # with h_in NULL it is the net's hidden row, which only the host has here
    rc.view(net.contents.hidden_layer, H)[1:40] = np.arange(39, dtype=np.float32)
    assert call(n=0, h_in=None) == 0
    assert np.array_equal(h_out[:, 1:40], np.tile(np.arange(39, dtype=np.float32), (w * h, 1)))
    for x in (bottom, two, net36, net):
        lib.rnn_delete_net(x)
