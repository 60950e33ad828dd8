"""Rate probe: what it costs to play rnnca's automaton, 144 x 96 cells (gstrnnca.h:14-15) under the default offset pattern
(35 inputs, 3 outputs), for 64 frames from a seed frame of random bytes.  Two forms, warmed up, alternated in the same run
and timed by the host clock around work that ends in a device synchronisation -- the caller's arrays made before the clock
starts:

  (a) today's loop, INTEGRATION.md section 3's recipe for fill_frame (gstrnnca.c:805-831): per frame the host gathers
      13,824 x 35 input floats from the frame before (numpy, the source cells worked out once), one rnn_amd_set_opinion
      over 13,824 forward-only clones uploads them and runs the pass, one rnn_amd_set_sigmoid_outputs brings 13,824 x 3
      floats back -- which synchronises --, and the host turns them into the next frame's bytes (numpy).  The host's share
      is the time of the gather and of the byte conversion, by the same clock, over the loop's time.
  (b) one rnn_amd_run_automaton for the 64 frames: at the default segment (16 MiB: 404 frames of this grid, so one segment
      here), at segments of 64 frames (one segment again, asked for by number) and of 1 frame (a copy and a
      synchronisation per frame).

The loops are driven from Python through ctypes, as every probe here is; clones and the set are made outside the clock.
At hidden 2048, then at hidden 512, seeded weights.  Figures are frames per second.

    python tools/gpu_automaton_rate.py [rounds]          # writes what profiles/r07_automaton_rate.txt holds
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import recur_ctypes as rc  # noqa: E402
from recur_amd.drivers import AutomatonGeometry, TRACE_GUARD, parse_offsets  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
WIDTH, HEIGHT, FRAMES = 144, 96, 64
SEGMENTS = [0, 64, 1]
F = np.float32


def sources(offsets, width, height):
    """the clamped source cell of every offset and cell (gstrnnca.c:644-667): [offsets][cells]"""
    cy, cx = np.divmod(np.arange(width * height), width)
    return np.array([np.clip(cy + dy, 0, height - 1) * width + np.clip(cx + dx, 0, width - 1) for dx, dy in offsets])


def main():
    amd = rc.load_amd()
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_automaton_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    ys, cs = parse_offsets(amd, "Y00120111C0111")
    geometry = AutomatonGeometry(WIDTH, HEIGHT, ys, cs, 2, 1)
    cells, inputs = WIDTH * HEIGHT, geometry.input_size
    index_y, index_c = sources(ys, WIDTH, HEIGHT), sources(cs, WIDTH, HEIGHT)
    ly, lc = len(ys), len(cs)
    cy, cx = np.divmod(np.arange(cells), WIDTH)
    position = np.stack([cx.astype(F) * F(1.0) / F(WIDTH), cy.astype(F) * F(1.0) / F(HEIGHT)], axis=1)
    recip = F(1.0) / F(255.0)
    seed = np.random.default_rng(7).integers(0, 256, (3, cells), dtype=np.uint8)
    print("workload: %d x %d = %d cells, %d inputs (%d Y and %d C offsets, 2 position inputs), 3 outputs, %d frames; a frame is "
          "%d bytes, a frame's inputs %d bytes, its answers %d bytes" % (WIDTH, HEIGHT, cells, inputs, ly, lc, FRAMES, 3 * cells,
                                                                          4 * cells * inputs, 4 * cells * 3))
    for hidden in (2048, 512):
        net = amd.rnn_new(inputs, hidden, 3, rc.FLAG_STANDARD, 11, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
        amd.rnn_randomise_weights_auto(net)
        O = net.contents.o_size
        flags = net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
        clones = (rc.NetP * cells)()
        for k in range(cells):
            clones[k] = amd.rnn_clone(net, flags, rc.SUBSEED, None)
        handle = amd.rnn_amd_set_open(clones, cells)
        assert handle
        rows = np.zeros((cells, inputs), F)
        rows[:, ly + 2 * lc:] = position
        out = np.zeros((cells, O), F)

        def loop(n_frames):
            """(a): returns (the frames, the loop's time, the host's time in it)"""
            frames = np.zeros((n_frames, 3, cells), np.uint8)
            before = seed
            amd.rnn_amd_synchronize()
            host = 0.0
            t0 = time.perf_counter()
            for t in range(n_frames):
                h0 = time.perf_counter()
                rows[:, :ly] = before[0][index_y].T.astype(F) * recip
                rows[:, ly:ly + 2 * lc:2] = before[1][index_c].T.astype(F) * recip
                rows[:, ly + 1:ly + 2 * lc:2] = before[2][index_c].T.astype(F) * recip
                host += time.perf_counter() - h0
                amd.rnn_amd_set_opinion(handle, rc.fptr(rows), inputs, None)
                amd.rnn_amd_set_sigmoid_outputs(handle, 3, rc.fptr(out))
                h0 = time.perf_counter()
                frames[t] = (out[:, :3] * F(255.9)).T.astype(np.uint8)   # (a sigmoid times 255.9 lies in [0, 256))
                before = frames[t]
                host += time.perf_counter() - h0
            amd.rnn_amd_synchronize()
            return frames, time.perf_counter() - t0, host

        def batched(segment):
            """(b): the frame array is the caller's and is made outside the clock, with guard bytes behind it"""
            frames = np.full(FRAMES * 3 * cells + TRACE_GUARD, 0xEE, np.uint8)
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            r = amd.rnn_amd_run_automaton(net, C.byref(geometry.struct), rc.u8ptr(seed), FRAMES, None, None, segment, rc.u8ptr(frames))
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            assert r == 0 and np.all(frames[FRAMES * 3 * cells:] == 0xEE)
            return frames[:FRAMES * 3 * cells].reshape(FRAMES, 3, cells), dt

        # warm-up: every kernel of both forms has run at its shapes.  The clones are fresh here (hidden rows zero, as the
        # net's), so the loop's first frames are the call's first frames up to the pixels whose level the two paths'
        # different kernel forms round apart; from then on the two runs are different films
        first, _, _ = loop(2)
        for segment in SEGMENTS:
            f_b, _ = batched(segment)
        same = float(np.mean(first[0] == f_b[0]))
        near = int(np.abs(first[0].astype(int) - f_b[0].astype(int)).max())
        t_a, h_a, t_b = [], [], {s: [] for s in SEGMENTS}
        for r in range(ROUNDS):
            _, dt, host = loop(FRAMES)
            t_a.append(dt)
            h_a.append(host)
            for segment in SEGMENTS:
                f_c, dt = batched(segment)
                t_b[segment].append(dt)
                assert np.array_equal(f_c, f_b)   # the segment size changes no bit, nor does the round
        ra = FRAMES / np.median(t_a)
        rbs = {s: FRAMES / np.median(t) for s, t in t_b.items()}
        print("hidden %4d: (a) today's loop, host gather + set_opinion + sigmoid_outputs + host bytes %7.1f frames/s (%s s); "
              "the host's share %.1f %% (%s s)" % (hidden, ra, " ".join("%.3f" % t for t in t_a),
                                                    100.0 * np.median(h_a) / np.median(t_a), " ".join("%.3f" % t for t in h_a)))
        for s in SEGMENTS:
            print("hidden %4d: (b) one rnn_amd_run_automaton, segment %-7s %7.1f frames/s (%s s)"
                  % (hidden, "default" if s == 0 else str(s), rbs[s], " ".join("%.4f" % t for t in t_b[s])))
        print("hidden %4d: (b default) / (a) = %.2f; %s" % (hidden, rbs[0] / ra, "; ".join(
            "segment %d / default = %.3f" % (s, rbs[s] / rbs[0]) for s in SEGMENTS[1:])))
        print("hidden %4d: frame 0 of (b) against frame 0 of (a): %.5f of the bytes the same, none further than %d level(s); the "
              "three segment sizes and every round give the same bits; %d levels in (b)'s last frame"
              % (hidden, same, near, len(np.unique(f_b[-1]))))
        amd.rnn_amd_set_close(handle)
        for k in range(cells - 1, -1, -1):
            amd.rnn_delete_net(clones[k])
        amd.rnn_delete_net(net)


if __name__ == "__main__":
    main()
