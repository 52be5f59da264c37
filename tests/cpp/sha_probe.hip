// sha_probe — the two-role SHA-256 routines of zkemail.rs_amd/csrc/sha256.hip.h alone on 1 024 messages of 4 KB (16 groups would
// be the benchmark's batch; 1 024 / 64 = 16 workgroups), timed, and — compiled with -DZKE_SHA_PROBE — with the routines' own
// record of where each wave ran and when it met each barrier.  Test infrastructure: compiled from the product header with the
// engine's flags (build.build_sha_probe), not part of the library.  tools/sha_timeline.py runs it once and prints the result.
//
//   sha_probe <report-out> [reps]          exit status: 0 done, 1 file error / digests differ, 2 HIP error
//
// Message i, byte j = (131 i + 7 j + (j >> 8)) & 255, so that whoever reads the report can hash the same bytes.
// Report, one record per line:
//   time <kernel> <median us> <min us> <reps>                    kernel = pair | ring
//   digest <kernel> <i> <hex>                                    messages 0, 1, 511, 1023 (all 1 024 are compared pair against ring here)
//   where <kernel | wgN> <group> <wave> <HW_ID hex> <XCC_ID hex> wgN: a workgroup of N threads with the pair routine's LDS
//   stamp <kernel> <role> <block> <point> <clock>                ZKE_SHA_PROBE builds only; role 0 feeder, 1 rounds; group 0
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "sha256.hip.h"

namespace {

constexpr uint32_t N = 1024, LEN = 4096, GROUPS = N / 64, T = 128;

// where the waves of an N-thread workgroup land: nothing but the registers
__global__ void where_kernel(uint32_t* out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  if ((threadIdx.x & 63) == 0) {
    uint32_t* o = out + (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
    o[0] = __builtin_amdgcn_s_getreg(4 | (31 << 11));
    o[1] = __builtin_amdgcn_s_getreg(20 | (31 << 11));
  }
  // stay for a while, so that the workgroups of the launch are resident together as the hash groups are
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  while (__builtin_amdgcn_s_memtime() - t0 < 20000) __builtin_amdgcn_s_sleep(8);
  if (threadIdx.x == 0xFFFF) lds_raw[0] = 1;
}

bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  fprintf(stderr, "sha_probe: %s: %s\n", what, hipGetErrorString(e));
  return false;
}

using Kernel = void (*)(const zke::ShaJob*, uint32_t);

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || argc > 3) { fprintf(stderr, "usage: sha_probe <report-out> [reps]\n"); return 1; }
  const int reps = argc == 3 ? std::max(1, std::min(1000, atoi(argv[2]))) : 50;
  FILE* rep = fopen(argv[1], "w");
  if (!rep) { fprintf(stderr, "sha_probe: cannot write %s\n", argv[1]); return 1; }

  std::vector<uint8_t> blob((size_t)N * LEN);
  for (uint32_t i = 0; i < N; i++)
    for (uint32_t j = 0; j < LEN; j++) blob[(size_t)i * LEN + j] = (uint8_t)(131 * i + 7 * j + (j >> 8));
  uint8_t *d_blob = nullptr, *d_dig = nullptr;
  zke::ShaJob* d_jobs = nullptr;
  uint32_t* d_where = nullptr;
  if (!hip_ok(hipMalloc(&d_blob, blob.size()), "hipMalloc") || !hip_ok(hipMalloc(&d_dig, 2 * N * 32), "hipMalloc") ||
      !hip_ok(hipMalloc(&d_jobs, 2 * N * sizeof(zke::ShaJob)), "hipMalloc") || !hip_ok(hipMalloc(&d_where, GROUPS * 4 * 2 * 4), "hipMalloc"))
    return 2;
  if (!hip_ok(hipMemcpy(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice), "upload")) return 2;
  std::vector<zke::ShaJob> jobs(2 * N);
  for (uint32_t k = 0; k < 2; k++)
    for (uint32_t i = 0; i < N; i++)
      jobs[k * N + i] = zke::ShaJob{(uint64_t)(uintptr_t)(d_blob + (size_t)i * LEN), (uint64_t)(uintptr_t)(d_dig + (size_t)(k * N + i) * 32), LEN, 0};
  if (!hip_ok(hipMemcpy(d_jobs, jobs.data(), jobs.size() * sizeof(zke::ShaJob), hipMemcpyHostToDevice), "upload")) return 2;

  const Kernel kernels[2] = {zke::sha256_pair_kernel<T>, zke::sha256_ring_kernel<T>};
  const size_t lds[2] = {zke::sha256_pair_lds_bytes<T>(), zke::sha256_ring_lds_bytes<T>()};
  const char* const names[2] = {"pair", "ring"};
  hipEvent_t e0, e1;
  if (!hip_ok(hipEventCreate(&e0), "event") || !hip_ok(hipEventCreate(&e1), "event")) return 2;
  for (int k = 0; k < 2; k++) {
    if (!hip_ok(hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[k]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds[k]), "attribute")) return 2;
    if (!hip_ok(hipMemset(d_dig + (size_t)k * N * 32, 0, N * 32), "hipMemset")) return 2;
    std::vector<float> us;
    for (int r = 0; r < reps + 3; r++) {                     // three launches to warm up
      if (!hip_ok(hipEventRecord(e0, 0), "record")) return 2;
      hipLaunchKernelGGL(kernels[k], dim3(GROUPS), dim3(128), lds[k], 0, d_jobs + (size_t)k * N, N);
      if (!hip_ok(hipGetLastError(), "launch") || !hip_ok(hipEventRecord(e1, 0), "record") || !hip_ok(hipEventSynchronize(e1), "run")) return 2;
      float ms = 0;
      if (!hip_ok(hipEventElapsedTime(&ms, e0, e1), "elapsed")) return 2;
      if (r >= 3) us.push_back(ms * 1000.f);
    }
    std::sort(us.begin(), us.end());
    fprintf(rep, "time %s %.2f %.2f %d\n", names[k], us[us.size() / 2], us[0], reps);
#ifdef ZKE_SHA_PROBE
    // the last launch's record
    static uint32_t hw[zke::SHA_PROBE_GROUPS][2][2];
    static unsigned long long stamp[2][zke::SHA_PROBE_BLKS][zke::SHA_PROBE_SLOTS];
    if (!hip_ok(hipMemcpyFromSymbol(hw, HIP_SYMBOL(zke::zke_sha_probe_hwid), sizeof hw), "symbol") ||
        !hip_ok(hipMemcpyFromSymbol(stamp, HIP_SYMBOL(zke::zke_sha_probe_stamp), sizeof stamp), "symbol"))
      return 2;
    for (uint32_t g = 0; g < GROUPS; g++)
      for (int w = 0; w < 2; w++) fprintf(rep, "where %s %u %d %08x %08x\n", names[k], g, w, hw[g][w][0], hw[g][w][1]);
    for (int w = 0; w < 2; w++)
      for (uint32_t b = 0; b < zke::SHA_PROBE_BLKS; b++)
        for (uint32_t p = 0; p < zke::SHA_PROBE_SLOTS; p++)
          if (stamp[w][b][p]) fprintf(rep, "stamp %s %d %u %u %llu\n", names[k], w, b + zke::SHA_PROBE_BLK0, p, stamp[w][b][p]);
    static const unsigned long long zero[2][zke::SHA_PROBE_BLKS][zke::SHA_PROBE_SLOTS] = {};
    if (!hip_ok(hipMemcpyToSymbol(HIP_SYMBOL(zke::zke_sha_probe_stamp), zero, sizeof zero), "symbol")) return 2;
#endif
  }
  std::vector<uint8_t> dig(2 * N * 32);
  if (!hip_ok(hipMemcpy(dig.data(), d_dig, dig.size(), hipMemcpyDeviceToHost), "copy back")) return 2;
  const bool same = memcmp(dig.data(), dig.data() + N * 32, N * 32) == 0;
  for (int k = 0; k < 2; k++)
    for (uint32_t i : {0u, 1u, 511u, 1023u}) {
      fprintf(rep, "digest %s %u ", names[k], i);
      for (int b = 0; b < 32; b++) fprintf(rep, "%02x", dig[(size_t)(k * N + i) * 32 + b]);
      fprintf(rep, "\n");
    }

  for (uint32_t threads : {128u, 192u, 256u}) {
    if (!hip_ok(hipMemset(d_where, 0, GROUPS * 4 * 2 * 4), "hipMemset")) return 2;
    hipLaunchKernelGGL(where_kernel, dim3(GROUPS), dim3(threads), lds[0], 0, d_where);
    if (!hip_ok(hipGetLastError(), "launch") || !hip_ok(hipDeviceSynchronize(), "run")) return 2;
    uint32_t w[GROUPS * 4 * 2];
    if (!hip_ok(hipMemcpy(w, d_where, sizeof w, hipMemcpyDeviceToHost), "copy back")) return 2;
    for (uint32_t g = 0; g < GROUPS; g++)
      for (uint32_t v = 0; v < threads / 64; v++) fprintf(rep, "where wg%u %u %u %08x %08x\n", threads, g, v, w[(g * 4 + v) * 2], w[(g * 4 + v) * 2 + 1]);
  }
  (void)hipFree(d_blob); (void)hipFree(d_dig); (void)hipFree(d_jobs); (void)hipFree(d_where);
  if (fclose(rep) != 0) { fprintf(stderr, "sha_probe: cannot write %s\n", argv[1]); return 1; }
  if (!same) { fprintf(stderr, "sha_probe: the two routines' digests differ\n"); return 1; }
  return 0;
}
