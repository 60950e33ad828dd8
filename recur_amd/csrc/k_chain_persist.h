// k_chain_persist.h -- the BPTT chain, one launch: k_chain_persist with its constants and its sync block (included by
// kernels_chain.hip, which launches it).  Its 256 workgroups wait for one another: residency, seats, the bounded poll and
// the give-up are k_coop.h's and are described in DESIGN.md, "Launches whose workgroups wait for one another".
//
// All D steps of the chain in ONE launch (hidden 1024: 32 column tiles; up to 8 row tiles of
// 32 streams).  What a kernel boundary costs the launch-per-step form -- 1.5 us of boundary,
// 1.7 us until the first operand stage has landed from a cold L2, the W panel fetched again
// every step -- is most of its 8.9 us; here the 32 workgroups that work on one row tile all
// run on ONE XCD (each reads the XCD it runs on from HW_REG_XCC_ID and draws its column tile
// by a ticket on that XCD: with one workgroup per CU and 32 CUs per XCD every XCD gets exactly
// 32, whatever the dispatch order), so that a step's output rows travel producer -> consumer
// through that XCD's L2 (plain stores, drained; a plain flag word per producer wave; L1-
// bypassing `sc1` polls and LDS-DMA loads), and each row tile is split into two independent
// sub-chains of 16 streams whose steps ALTERNATE on the matrix pipe: while the 32 workgroups
// exchange sub-chain a's step t, they multiply sub-chain b's.  (A row tile's recurrences are
// independent per stream: E[t+1][s] = mask[t][s] . (E[t][s] W^T), recur-nn.c:338-376.)
//
// Workgroup = 8 waves.  Waves 4-7 (one per SIMD) only multiply: the workgroup's W panel
// (32 output columns x 1024 k) lives in their registers for the whole launch as MFMA B
// fragments (v_mfma_f32_16x16x4_f32; each wave a quarter of K: 128 VGPRs), the A operand --
// 16 error rows x 1024 k per sub-chain, 64 KB -- is read from LDS with conflict-free
// ds_read_b128 (16-byte chunk c of row m sits at position c ^ m).  Waves 0-3 do everything
// else for four of the 16 rows each: finish the previous half-step (sum the four K quarters
// from LDS, zero-row mask, RESQRT derivative, sum of squares, store the rows), publish, poll
// the 32 producers of their rows, and pull the next operand into LDS by LDS-DMA.  One
// s_barrier per half-step couples the two groups.  Every poll is bounded; a time-out or a
// surplus ticket raises the abort word (host-mapped), which the library checks at its next
// synchronisation and aborts on -- results are never silently wrong.
/* (PC_SUB, the streams per sub-chain, PC_RED_FLOATS and pc_lds_bytes: k_tiles.h -- the residency probe has the launch's footprint) */
/* s_sleep units (64 cycles) between the barrier and the first poll; the producers publish ~0.35 us after
 * the barrier and the flag is visible in the XCD's L2 ~0.2 us later.  Round 3 (20 steps of 1024 / 256,
 * us per chain): first poll after 16 / 18 / 22 / 24 / 26 / 32 units with gaps from K block 3 on =
 * 114 / 105 / 100.6 / 100.7 / 101.3 / 105. */
#ifndef PC_SLEEP0
#define PC_SLEEP0 22
#endif
#ifndef PC_SLEEP0_ONE
#define PC_SLEEP0_ONE 12 /* 16-stream row tiles: the publish comes in an otherwise empty half-step */
#endif
#ifndef PC_SLEEP0_SMALL
#define PC_SLEEP0_SMALL 14 /* hidden 512 / 256: the half-step is shorter, the publish comes at the same ~0.35 us */
#endif
constexpr unsigned PC_EPOCH = COOP_CHAIN_EPOCH; /* flag values per launch (depth <= 60) */
/* K blocks (8 MFMAs each) after which the multiplying waves pause for 64 cycles, per hidden size:
 * measured at 1024: after blocks 3-6 100.6 us per chain, 3-7 100.8, 4-7 100.7, 3-8 100.9, 2-6 105.5,
 * 2-9 104.6, every block from 3 on 109.9, blocks 5 / 7 / 9 / 11 103.6-105.1, none (the poll then
 * completes when the burst has ended) 133. */
#ifndef PC_GAPS
#define PC_GAPS 0x78
#endif
/* The early form (EARLY below: K block 0 stands in front of the flag) has its own two constants: by the stamped workgroup's
 * marks (profiles/r20_chain_early_stamps_*.txt, means of 37 half-steps) its flag comes 0.03 us later (rows stored -> flag 0.146
 * -> 0.177 us) and the burst behind it ends 0.10 us earlier (flag -> burst end 1.977 -> 1.874), and with k_chain_persist's
 * constants it is SLOWER.  Round 20, 1024 / 256 /
 * 20, us per generation (k_chain_persist 206.1-206.6; with pauses after blocks 4-7 206.5-206.7: no gain of its own):
 *   EARLY 1 / 2 / 3 with pauses after blocks 3-6, first poll after 22 units: 211.8-212.6 / 215.8-216.4 / 221.2-221.6;
 *   EARLY 1, pauses after 4-7, first poll after 18 / 20 / 21 / 22 / 23 / 24: 205.4-206.1 / 204.1-204.7 / 204.0-204.1 /
 *     203.6-204.3 / 203.3-204.0 / 207.8-208.5;
 *   EARLY 1, first poll after 22, pauses after 2-5 / 4-6 / 5-7 / 5-8 / 4-8 / 3-7: 218.0-218.9 / 204.4-205.5 / 204.9-205.0 /
 *     204.5-205.1 / 205.2-205.6 / 210.9-211.4;
 *   EARLY 2, pauses after 4-7 / 5-8 / 4-8: 207.1-207.7 / 205.7-205.8 / 207.1-207.2.  (profiles/NOTES_r20.md) */
#ifndef PC_GAPS_EARLY
#define PC_GAPS_EARLY 0xf0
#endif
#ifndef PC_SLEEP0_EARLY
#define PC_SLEEP0_EARLY 22
#endif
#ifndef PC_GAPS_512
#define PC_GAPS_512 0x3c
#endif
#ifndef PC_GAPS_256
#define PC_GAPS_256 0xe
#endif
/* (Tried as build switches and retired, none faster: foreign MFMAs in the drain window -- profiles/r03_fused_delta_negative.txt;
 * a scalar poll of the flag words, s_nop gaps instead of s_sleep, s_setprio 3 around the fetch, ONE's fetching waves
 * fetching all of their rows themselves -- profiles/NOTES_r01_r03_design_diary.md, round 3, "133 -> 100.6 us".) */

struct ChainSync {
  unsigned tickets[8];       /* per XCD, monotonic over launches                     */
  unsigned pad0[24];
  unsigned flags[32][2][4][32]; /* [row tile][sub-chain][fetching wave][column tile]   */
  unsigned abort;            /* raised by any workgroup that gives up                */
};

#ifdef PC_STAMPS /* development builds only (tools/mkabl.sh -DPC_STAMPS): where a half-step's time goes */
__device__ unsigned long long g_pc_stamps[2][64][8];
#define PC_STAMP(role, k, slot)                                                                    \
  do {                                                                                             \
    if (g == 0 && j == 0 && lane == 0 && (wave8 & 3) == 0 && (k) < 64)                             \
      g_pc_stamps[role][k][slot] = __builtin_amdgcn_s_memrealtime();                               \
  } while (0)
#else
#define PC_STAMP(role, k, slot) do { } while (0)
#endif

/* The top layer's weight delta in the chain launch's first microseconds (HoWork, k_common.h): 22 MFLOP that as
 * a launch of their own (k_gemm<ProbHoDelta>) cost 6 us of launch, ramp and three dependent memory round trips
 * on the generation's critical path.  Here the launch's workgroups share the rows of the delta, HR =
 * ceil(H / workers) each: all 256 of them before they request their weight panel / while their first operand
 * rows are in flight, or -- when at least half of the launch has no chain work, a small set -- only those
 * (hw.idle_only; the others start their chain at once).  Lane (output quad q4, group gl) of wave w sums
 * streams g = 4 w + gl, g + 32, ... for ALL HR rows: one float4 of o_error and HR hidden values per stream (a
 * thread per row instead had five lanes load every float4 again, and the texture path is paid by the lane:
 * 3.6 us, now 2.5).  The four groups of a wave are added by shuffles, the eight waves in order through LDS
 * (`lds`: 8 x HO_HR x 64 floats the caller does not need yet: the partial-tile area, which is unused until the
 * first multiply has finished, or the operand buffers of a workgroup without chain work).  A workgroup's 512
 * threads all call it, once (two barriers). */
/* (chain_ho_sum / chain_ho_delta: k_common.h -- the weight-delta launch of the fused text step runs them too) */
/* ONE: row tiles of 16 streams, i.e. only sub-chain a exists and every other half-step is empty
 * (the workgroup multiplies, then finishes and publishes, then waits for the 32 producers of its
 * next operand): 4.5 instead of 6.4 us per step for HALF the streams per workgroup -- worse per
 * stream, but a small set (64 streams at hidden 1024: a GPU's share of 512 on eight) then runs
 * on twice as many CUs.  The launcher picks it when the 16-stream tiles still fit one launch. */
/* PAD (with ONE): the set is not whole row tiles -- only rows [vlo, nvalid) of the launch are its
 * own; the others belong to other streams or to nobody: they are multiplied like the rest (rows
 * do not mix) and never stored. */
/* EARLY: the K blocks (8 MFMAs each) of a half-step's burst that the multiplying waves issue between the finish's row
 * stores and the drain that waits for their acknowledgement (round 20; the comment at the drain has the numbers).  Block 0
 * needs nothing the drain waits for -- its A fragments landed behind the finish's lgkmcnt(0), the panel is resident, the
 * accumulators start at zero -- and the MFMA order into acc0 / acc1 is the same, so results are bit for bit EARLY = 0's.
 * 0 in k_chain_persist, whose instantiations stay what they were instruction for instruction (this kernel's loop has moved
 * three times because of code that was never executed); k_chain_persist_early is the kernel of its own that has it. */
template <int ACT, int K, bool ONE = false, bool PAD = false, bool XD = false> /* rnn_activation; hidden size: 1024, 512 or 256; XD: the tail for DENSE inputs (an instantiation of its own: the text step's kernel stays what it is) */
__global__ __launch_bounds__(512) void k_chain_persist(const View *__restrict__ vp, int uniform_idx,
                                                       int row0, int nrows, int depth, unsigned seq,
                                                       ChainSync *sy, unsigned *host_abort, int nvalid, int vlo,
                                                       HoWork hw, XcWork xc, int static_map, unsigned tseq, const unsigned *seats) {
  constexpr int EARLY = 0;
#include "k_chain_persist_body.h"
}
/* hidden 1024, 32-stream row tiles, the text step's tail: the only shape chain_plan.h (chain_early_blocks) asks it for */
template <int ACT, int EARLY>
__global__ __launch_bounds__(512) void k_chain_persist_early(const View *__restrict__ vp, int uniform_idx,
                                                             int row0, int nrows, int depth, unsigned seq,
                                                             ChainSync *sy, unsigned *host_abort, int nvalid, int vlo,
                                                             HoWork hw, XcWork xc, int static_map, unsigned tseq, const unsigned *seats) {
  constexpr int K = 1024;
  constexpr bool ONE = false, PAD = false, XD = false;
  static_assert(EARLY > 0 && EARLY < K / 64, "some of the burst stays behind the flag");
#include "k_chain_persist_body.h"
}
