// sha_twin_probe — sha256_ring_kernel against sha256_twin_kernel (zkemail.rs_amd/csrc/sha256.hip.h) alone on 1 024 messages of
// 4 KB: 16 ring groups of 64 messages, 32 twin groups of 32.  The companion of sha_probe.hip (which stays with the pair and the
// ring): the same messages, the same report format, the same two builds — with -DZKE_SHA_PROBE the routines record where their
// waves ran and when they met each barrier.  Test infrastructure: compiled from the product header with the engine's flags
// (build.build_sha_twin_probe), not part of the library.  tools/sha_twin_timeline.py runs it once and prints the result.
//
//   sha_twin_probe <report-out> [reps]     exit status: 0 done, 1 file error / digests differ, 2 HIP error
//
// Message i, byte j = (131 i + 7 j + (j >> 8)) & 255.  Report, one record per line:
//   time <kernel> <median us> <min us> <reps>                    kernel = ring | twin
//   digest <kernel> <i> <hex>                                    messages 0, 1, 31, 32, 511, 1023 (all 1 024 are compared here)
//   stamp <kernel> <role> <block> <point> <clock>                ZKE_SHA_PROBE builds only; role 0 feeder, 1 rounds; group 0.
//                                                                The twin's feeder stamps its passes: even blocks only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "sha256.hip.h"

namespace {

constexpr uint32_t N = 1024, LEN = 4096, T = 128;

bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  fprintf(stderr, "sha_twin_probe: %s: %s\n", what, hipGetErrorString(e));
  return false;
}

using Kernel = void (*)(const zke::ShaJob*, uint32_t);

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || argc > 3) { fprintf(stderr, "usage: sha_twin_probe <report-out> [reps]\n"); return 1; }
  const int reps = argc == 3 ? std::max(1, std::min(1000, atoi(argv[2]))) : 50;
  FILE* rep = fopen(argv[1], "w");
  if (!rep) { fprintf(stderr, "sha_twin_probe: cannot write %s\n", argv[1]); return 1; }

  std::vector<uint8_t> blob((size_t)N * LEN);
  for (uint32_t i = 0; i < N; i++)
    for (uint32_t j = 0; j < LEN; j++) blob[(size_t)i * LEN + j] = (uint8_t)(131 * i + 7 * j + (j >> 8));
  uint8_t *d_blob = nullptr, *d_dig = nullptr;
  zke::ShaJob* d_jobs = nullptr;
  if (!hip_ok(hipMalloc(&d_blob, blob.size()), "hipMalloc") || !hip_ok(hipMalloc(&d_dig, 2 * N * 32), "hipMalloc") ||
      !hip_ok(hipMalloc(&d_jobs, 2 * N * sizeof(zke::ShaJob)), "hipMalloc"))
    return 2;
  if (!hip_ok(hipMemcpy(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice), "upload")) return 2;
  std::vector<zke::ShaJob> jobs(2 * N);
  for (uint32_t k = 0; k < 2; k++)
    for (uint32_t i = 0; i < N; i++)
      jobs[k * N + i] = zke::ShaJob{(uint64_t)(uintptr_t)(d_blob + (size_t)i * LEN), (uint64_t)(uintptr_t)(d_dig + (size_t)(k * N + i) * 32), LEN, 0};
  if (!hip_ok(hipMemcpy(d_jobs, jobs.data(), jobs.size() * sizeof(zke::ShaJob), hipMemcpyHostToDevice), "upload")) return 2;

  const Kernel kernels[2] = {zke::sha256_ring_kernel<T>, zke::sha256_twin_kernel<T>};
  const uint32_t groups[2] = {N / 64, N / zke::SHA_TWIN_WIDTH};
  const size_t lds = zke::sha256_ring_lds_bytes<T>();
  const char* const names[2] = {"ring", "twin"};
  hipEvent_t e0, e1;
  if (!hip_ok(hipEventCreate(&e0), "event") || !hip_ok(hipEventCreate(&e1), "event")) return 2;
  for (int k = 0; k < 2; k++) {
    if (!hip_ok(hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[k]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "attribute")) return 2;
    if (!hip_ok(hipMemset(d_dig + (size_t)k * N * 32, 0, N * 32), "hipMemset")) return 2;
    std::vector<float> us;
    for (int r = 0; r < reps + 3; r++) {                     // three launches to warm up
      if (!hip_ok(hipEventRecord(e0, 0), "record")) return 2;
      hipLaunchKernelGGL(kernels[k], dim3(groups[k]), dim3(128), lds, 0, d_jobs + (size_t)k * N, N);
      if (!hip_ok(hipGetLastError(), "launch") || !hip_ok(hipEventRecord(e1, 0), "record") || !hip_ok(hipEventSynchronize(e1), "run")) return 2;
      float ms = 0;
      if (!hip_ok(hipEventElapsedTime(&ms, e0, e1), "elapsed")) return 2;
      if (r >= 3) us.push_back(ms * 1000.f);
    }
    std::sort(us.begin(), us.end());
    fprintf(rep, "time %s %.2f %.2f %d\n", names[k], us[us.size() / 2], us[0], reps);
#ifdef ZKE_SHA_PROBE
    static unsigned long long stamp[2][zke::SHA_PROBE_BLKS][zke::SHA_PROBE_SLOTS];      // the last launch's record
    if (!hip_ok(hipMemcpyFromSymbol(stamp, HIP_SYMBOL(zke::zke_sha_probe_stamp), sizeof stamp), "symbol")) return 2;
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
    for (uint32_t i : {0u, 1u, 31u, 32u, 511u, 1023u}) {
      fprintf(rep, "digest %s %u ", names[k], i);
      for (int b = 0; b < 32; b++) fprintf(rep, "%02x", dig[(size_t)(k * N + i) * 32 + b]);
      fprintf(rep, "\n");
    }
  (void)hipFree(d_blob); (void)hipFree(d_dig); (void)hipFree(d_jobs);
  if (fclose(rep) != 0) { fprintf(stderr, "sha_twin_probe: cannot write %s\n", argv[1]); return 1; }
  if (!same) { fprintf(stderr, "sha_twin_probe: the two routines' digests differ\n"); return 1; }
  return 0;
}
