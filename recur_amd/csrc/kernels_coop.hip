// kernels_coop.hip -- the process state of the launches whose 256 workgroups wait for one another, one per CU (the
// one-launch BPTT chain k_chain_persist, the text step's forward + top launch k_fwd_top; DESIGN.md, "Launches whose
// workgroups wait for one another"): the residency probe, run once, what it found (coop_rule.h reads it), the seat table
// on the device, and the host-mapped abort word that every bounded device-side wait of the library raises.
#include "k_coop.h"

/* Such a launch needs all 256 workgroups resident together, one per CU.  Whether this process's device and queue grant
 * that -- no CU mask, no partition mode that still reports 256 CUs, no co-tenant holding CUs -- is found out ONCE, by a
 * probe launch of the one-launch chain's footprint (512 threads and pc_lds_bytes(1024) per workgroup, so one per CU)
 * whose workgroups count themselves and wait, bounded, for the count to reach 256.  It also records the XCD and the CU
 * each workgroup found itself on: the seat table, and whether the dispatcher deals workgroups to the XCDs in turn.  A
 * probe that fails switches these launches off for the process; the launch-per-step chain and the two launches of the
 * text step take their place from the first call on.  A give-up in mid-run -- a co-tenant that arrives later -- is
 * caught at the next synchronisation (engine.c: ramd_dsync). */
__global__ __launch_bounds__(512) void k_residency_probe(CoopProbe *p) {
  extern __shared__ float probe_lds[]; /* (sized by the launch: what makes it one workgroup per CU) */
  if (threadIdx.x != 0) return;
  p->xcc[blockIdx.x] = coop_hw_xcc();
  p->cu_key[blockIdx.x] = PC_HW_CU_KEY();
  __hip_atomic_fetch_add(&p->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (unsigned spins = 0; __hip_atomic_load(&p->arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x; spins++) {
    if (spins > (1u << 20) || __hip_atomic_load(&p->fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { /* ~0.5 s */
      __hip_atomic_store(&p->fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    __builtin_amdgcn_s_sleep(8);
  }
}

static bool g_validated = false, g_broken = false, g_in_turn = false, g_seat_table = false;
static unsigned *g_seats = nullptr; /* SeatTable, device */
/* Another queue of this process may have work on the device beside the main one (the noise generated ahead on a side
 * stream, an exchange overlapped on a communication stream): the dispatcher then deals the workgroups of BOTH launches
 * to the XCDs in turn, and workgroup i of the chain is not on XCD i % 8 (found by the configs[3] test, whose every
 * wave's check raised the abort word).  The host code says so when it creates such a stream; from then on the chain
 * does not take its seats from the workgroup number, and the forward + top launch is not taken. */
static bool g_side_streams = false;
extern "C" void ramd_note_side_stream(void) { g_side_streams = true; }

/* the probe, once per process */
static void coop_validate(hipStream_t st) {
  if (g_validated || g_broken) return;
  int dev = 0, cus = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  if (cus != COOP_WGS) { /* 8 XCDs x 32 CUs: one workgroup per CU, 32 seats per XCD */
    g_broken = true;
    return;
  }
  CoopProbe *d_probe = nullptr, h_probe;
  HIP_CHECK(hipMalloc(&d_probe, sizeof(CoopProbe)));
  HIP_CHECK(hipMemsetAsync(d_probe, 0, sizeof(CoopProbe), st));
  HIP_CHECK(hipFuncSetAttribute((const void *)k_residency_probe, hipFuncAttributeMaxDynamicSharedMemorySize, pc_lds_bytes(1024)));
  RAMD_LAUNCH(k_residency_probe, dim3(COOP_WGS), dim3(512), pc_lds_bytes(1024), st, d_probe);
  HIP_CHECK(hipMemcpyAsync(&h_probe, d_probe, sizeof(CoopProbe), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipFree(d_probe));
  /* (RECUR_AMD_CHAIN_TEST_GIVEUP=1: the tests' way of taking the failure branch on a healthy device) */
  if (!coop_resident(&h_probe) || env_int("RECUR_AMD_CHAIN_TEST_GIVEUP", 0) == 1) {
    fprintf(stderr, "librecur_amd: the residency probe failed (%u of 256 workgroups resident together, one per CU); "
                    "using the launch-per-step chain from here on\n", h_probe.arrived);
    g_broken = true;
    return;
  }
  g_in_turn = coop_in_turn(&h_probe);
  static SeatTable h_seats;
  g_seat_table = coop_seat_table(&h_probe, &h_seats) && env_int("RECUR_AMD_XCD_TABLE", 1);
  if (g_seat_table) {
    if (!g_seats) HIP_CHECK(hipMalloc(&g_seats, sizeof(SeatTable)));
    HIP_CHECK(hipMemcpy(g_seats, &h_seats, sizeof(SeatTable), hipMemcpyHostToDevice));
  }
  g_validated = true;
}

SeatRule coop_seat_rule(hipStream_t st) {
  coop_validate(st);
  return SeatRule{g_validated && !g_broken, g_seat_table, g_side_streams,
                  coop_seat_mode(g_seat_table, env_int("RECUR_AMD_XCD_STATIC", 0), g_in_turn, g_side_streams), g_seats};
}

/* the host-mapped abort word and its device address, for every bounded device-side wait (the exchange's barriers too) */
static unsigned *g_abort_host = nullptr, *g_abort_dev = nullptr;
extern "C" unsigned *ramd_abort_word_dev(void) {
  if (!g_abort_host) {
    HIP_CHECK(hipHostMalloc((void **)&g_abort_host, 64, hipHostMallocMapped));
    *g_abort_host = 0;
    HIP_CHECK(hipHostGetDevicePointer((void **)&g_abort_dev, g_abort_host, 0));
  }
  return g_abort_dev;
}
extern "C" unsigned ramd_chain_abort_word(void) { return g_abort_host ? *(volatile unsigned *)g_abort_host : 0u; }

void coop_mark_broken(void) {
  if (g_abort_host) *(volatile unsigned *)g_abort_host = 0;
  g_broken = true;
}
