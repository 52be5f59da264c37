// sha256.hip.h — batched SHA-256 for gfx950 (CDNA4).  FIPS 180-4.
//
// Replaces sha2 0.10.9 on the verify path: hash_bytes (core/src/crypto.rs:3-7, used at
// core/src/circuits.rs:16-17) and the body / header hashes inside cfdkim
// (call site core/src/email.rs:31-33).
//
// Mapping.  SHA-256 is a strictly sequential chain per message, so parallelism comes
// from the batch: ONE MESSAGE PER LANE for the compression (64 messages per wavefront,
// all 64 lanes doing integer VALU work), while the bytes are fetched WAVE-COOPERATIVELY:
// for each tile of T bytes the 64 lanes read each message's tile with 16-byte
// lane-contiguous global loads (T/16 lanes cover one message's tile -> T-byte contiguous
// segments; the engine compiles T = SHA_TILE = 128: 8 lanes per message, two SHA blocks
// per tile), park it in the wave's private LDS slab, and every lane
// then pulls its own message's 64-byte blocks back with ds_read_b128.  Row stride T+16
// bytes keeps both the ds_write_b128 and the ds_read_b128 phases conflict-free
// (lane stride = 4 banks mod 64).  No __syncthreads in the staging: a wave's LDS operations
// execute in order, and no other wave touches its slab.
//
// Roofline: integer-VALU bound (about 1.4k VALU per 64-byte block per lane), not HBM
// bound; DESIGN.md §3 has the arithmetic.
//
// Four routines, each its own control flow over the shared pieces below:
//   sha256_batch_kernel  one wave per 64 messages, for launches that fill the chip;
//   sha256_pair_group    two waves per 64 messages — message schedule and rounds —, ONE K+W buffer and two barriers per
//                        block, 28 KB of LDS: for launches whose duration is one wave's chain of compressions, where
//                        many batches share the chip.  Its one-wave path takes the groups that hold a SHA-1 job;
//   sha256_ring_group    the same two roles, TWO K+W buffers and one LDS-only barrier per block, 45 KB: where few batches
//                        are on the chip (engine.hip chooses);
//   sha256_twin_group    the ring with 32 messages per group and TWO LANES PER MESSAGE in the rounds wave (e..h in one, a..d in
//                        its partner, exchanged by DPP): 10 instead of 14 instructions per round on the chain, two blocks per
//                        feeder pass, one barrier per pass.  The ring's LDS; taken with the ring, for messages of many blocks.
// The group routines are device functions, so that other work can share their launch (fused.hip.h); sha256_pair_kernel,
// sha256_ring_kernel and sha256_twin_kernel run them alone.
// Shared, one definition each: the round constants SHA_K; sha_init_state / sha_store_digest (sha_lane of verdict.hip.h
// uses them too); sha_load_block; ShaLaneJob (a lane's job, the wave's longest message, its SHA-1 ballot); ShaTile
// (descriptor rows, fetch / commit: tile staging and padding); sha_one_wave_tiles (the one-wave tile loop);
// sha_group_pick (the length-bucket protocol of a two-wave group); sha_kw_schedule and sha_rounds_kw (the two halves of
// a split compression).  The pair, the ring and the twin block loops are NOT shared: they differ in their barrier structure,
// and that difference is what a reader has to see.  The ring and the twin also keep their 64 rounds written out, for a
// measured reason (the comment in the ring).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage_plan.hip.h"      // SHA_TWIN_WIDTH: a group's width is part of the launch layout

// A message is a serial chain of compressions, so a hash launch's duration is set by its longest message, not by
// the chip: with several batches in flight its few waves share SIMDs with thousands of front-end / RSA waves and
// the chain stretches ~2x.  Raising the wave priority keeps the chain near its unloaded latency; the other
// kernels have parallel slack to absorb it.
#ifndef ZKE_SHA_PRIO
#define ZKE_SHA_PRIO 3
#endif

namespace zke {

struct ShaJob {          // one message
  uint64_t src;          // device address of the bytes
  uint64_t dst;          // device address of the 32-byte digest slot (0 = inactive job)
  uint32_t len;          // bytes
  uint32_t pad;          // 0: SHA-256; 1: SHA-1 (a=rsa-sha1 signatures; 20-byte digest, slot zero padded)
};

// ---- length buckets --------------------------------------------------------------------------------------------------
// A wave hashes 64 messages in lock-step: it runs as many compressions as its LONGEST message needs.  In a ragged batch
// (body lengths log-uniform over 0 .. 64 KB) 64 messages in arrival order span the whole range, so most lanes of
// most waves idle for most of the launch.  The front end therefore files every body (and header preimage) under a length
// class — its block count to three significant bits — with one atomic add: key[i] = class << 24 | position within the class.
// A hash group lays the classes out longest first (a prefix sum over the 192 counters), finds the 64 messages whose global
// position falls into its range by one pass over the keys, and hashes messages of one class: no wave waits for a message more
// than 12.5 % longer than its shortest.  No sort, no extra launch; the digests land by ShaJob::dst, so record order is untouched.
// Batches whose messages all fall into one or two neighbouring classes (the uniform BASELINE configs) keep the direct
// mapping lane -> job: the pass over the keys is skipped.
constexpr uint32_t SHA_CLASSES = 192;               // block counts 1..15 exactly, then 8 classes per octave up to 2^25 blocks
constexpr uint32_t SHA_ORDER_KIND_WORDS = 256;      // counters of one kind (192 used).  The slot's order buffer: the counters of kind 0,
                                                    // those of kind 1 — at fixed places, whatever the batch size: they carry over from
                                                    // batch to batch —, then n_pad keys of kind 0, n_pad keys of kind 1
__host__ __device__ inline size_t sha_order_cnt(uint32_t kind) { return (size_t)kind * SHA_ORDER_KIND_WORDS; }
__host__ __device__ inline size_t sha_order_key(uint32_t kind, uint32_t n_pad) { return 2 * (size_t)SHA_ORDER_KIND_WORDS + (size_t)kind * n_pad; }
constexpr uint32_t SHA_KEY_NONE = 0xFFFFFFFFu;
__host__ __device__ inline uint32_t sha_len_class(uint32_t nblk) {
  if (nblk < 16) return nblk;
  const uint32_t e = 31u - (uint32_t)__builtin_clz(nblk);                  // >= 4
  return 16u + (e - 4u) * 8u + ((nblk >> (e - 3u)) & 7u);
}
struct ShaOrder {                 // one kind's part of the slot's order buffer (nullptr cnt: no buckets, direct mapping)
  const uint32_t* cnt;            // [SHA_CLASSES] messages per class
  const uint32_t* key;            // [n] class << 24 | position, SHA_KEY_NONE for an e-mail without a message of this kind
  uint32_t n;                     // e-mails
};

// ---- one compression and its pieces ----------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rotr32(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
// gfx950 v_bitop3_b32: any 3-input boolean function in one VALU op (truth table in the immediate)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ uint32_t ch3(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA); }   // e ? f : g
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }

// The round constants: compile-time literals after full unrolling (no loads), in sha256_compress and in sha_kw_schedule.
constexpr uint32_t SHA_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

// One compression.  w[16] holds the big-endian message words and is consumed.
__device__ __forceinline__ void sha256_compress(uint32_t (&st)[8], uint32_t (&w)[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    uint32_t wi;
    if (i < 16) {
      wi = w[i];
    } else {
      uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
      uint32_t s0 = xor3(rotr32(w15, 7), rotr32(w15, 18), w15 >> 3);
      uint32_t s1 = xor3(rotr32(w2, 17), rotr32(w2, 19), w2 >> 10);
      wi = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
      w[i & 15] = wi;
    }
    uint32_t S1 = xor3(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25));
    uint32_t t1 = (h + S1 + ch3(e, f, g)) + (SHA_K[i] + wi);
    uint32_t S0 = xor3(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22));
    uint32_t mj = maj3(a, b, c);
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// SHA-1 (FIPS 180-4 §6.1), same block size and padding as SHA-256; used only for a=rsa-sha1 signatures
// (cfdkim HashAlgo::RsaSha1 over sha-1 0.10.1).
__device__ __forceinline__ void sha1_compress(uint32_t (&st)[8], uint32_t (&w)[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
#pragma unroll
  for (int i = 0; i < 80; i++) {
    uint32_t wi;
    if (i < 16) {
      wi = w[i];
    } else {
      const uint32_t x = xor3(w[(i - 3) & 15], w[(i - 8) & 15], w[(i - 14) & 15]) ^ w[i & 15];
      wi = rotr32(x, 31);
      w[i & 15] = wi;
    }
    uint32_t f, k;
    if (i < 20) { f = ch3(b, c, d); k = 0x5A827999u; }
    else if (i < 40) { f = xor3(b, c, d); k = 0x6ED9EBA1u; }
    else if (i < 60) { f = maj3(b, c, d); k = 0x8F1BBCDCu; }
    else { f = xor3(b, c, d); k = 0xCA62C1D6u; }
    const uint32_t t = rotr32(a, 27) + f + e + (k + wi);
    e = d; d = c; c = rotr32(b, 2); b = a; a = t;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e;
}

// The initial chaining state.  sha1: ShaJob::pad != 0 (SHA-1: five words, the other three idle at zero).
__device__ __forceinline__ void sha_init_state(uint32_t (&st)[8], bool sha1) {
  st[0] = 0x6a09e667; st[1] = 0xbb67ae85; st[2] = 0x3c6ef372; st[3] = 0xa54ff53a;
  st[4] = 0x510e527f; st[5] = 0x9b05688c; st[6] = 0x1f83d9ab; st[7] = 0x5be0cd19;
  if (sha1) { st[0] = 0x67452301; st[1] = 0xEFCDAB89; st[2] = 0x98BADCFE; st[3] = 0x10325476; st[4] = 0xC3D2E1F0; st[5] = st[6] = st[7] = 0; }
}

// The digest into its 32-byte slot, big-endian; a SHA-1 digest is 20 bytes and the slot's rest zero.  Out: the caller's
// pointer type, so that the stores stay in its address space (gptr_out32: global_store; sha_lane's plain pointer: as it was).
template <class Out>
__device__ __forceinline__ void sha_store_digest(Out out, const uint32_t (&st)[8], bool sha1) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = (sha1 && i >= 5) ? 0u : __builtin_bswap32(st[i]);
}

// A 64-byte block (16-byte aligned; the routines read their LDS rows: four ds_read_b128) as the 16 big-endian words.
__device__ __forceinline__ void sha_load_block(uint32_t (&w)[16], const uint8_t* block) {
  const uint4* src = (const uint4*)block;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint4 v = src[q];
    w[4 * q + 0] = __builtin_bswap32(v.x); w[4 * q + 1] = __builtin_bswap32(v.y);
    w[4 * q + 2] = __builtin_bswap32(v.z); w[4 * q + 3] = __builtin_bswap32(v.w);
  }
}

// ---- a lane's job, the tile staging ----------------------------------------------------------------------------------
typedef uint4 __attribute__((aligned(1))) uint4_unaligned;
// Message bytes are in HBM, but their addresses arrive as integers (ShaJob::src), so the compiler would emit FLAT
// loads: those count on lgkmcnt as well as vmcnt, and every wait for an LDS read behind one (the next row's
// descriptor) then waits for HBM too — a tile's loads went out one at a time.  Typed as address space 1 they are
// global_load_*: all of a tile's loads are in flight together and only commit() waits for them.
typedef uint32_t u32x4_raw __attribute__((ext_vector_type(4)));          // a plain vector: the host pass cannot bind HIP's uint4 class across address spaces
typedef const u32x4_raw __attribute__((aligned(1), address_space(1)))* gptr_u4;
typedef const uint8_t __attribute__((address_space(1)))* gptr_u8;
typedef uint32_t __attribute__((address_space(1)))* gptr_out32;         // digests are 4-byte aligned (result records / engine buffers)

// Job m of `jobs` as the lane that hashes it holds it (m >= n, or dst == 0 for an inactive job: nothing to do, nblk 0).
struct ShaLaneJob {
  uint64_t src = 0, dst = 0;
  uint32_t len = 0, nblk = 0, algo = 0;
  __device__ __forceinline__ ShaLaneJob(const ShaJob* __restrict__ jobs, uint32_t m, uint32_t n) {
    if (m < n) {
      ShaJob j = jobs[m];
      src = j.src; dst = j.dst; len = j.len; algo = j.pad;
      nblk = dst ? (len + 9 + 63) >> 6 : 0;
    }
  }
  // wave-uniform: the blocks of the wave's longest message
  __device__ __forceinline__ uint32_t wave_max_nblk() const {
    uint32_t max_nblk = nblk;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) max_nblk = max(max_nblk, (uint32_t)__shfl_xor((int)max_nblk, o));
    return __builtin_amdgcn_readfirstlane(max_nblk);
  }
  // wave-uniform: SHA-256-only waves skip the SHA-1 code
  __device__ __forceinline__ bool wave_any_sha1() const { return __ballot(algo != 0) != 0; }
};

// The tile staging of one wave's 64 messages.  LDS at `slab`: 64 rows of T + 16 bytes, then 64 descriptors of 16 bytes.
// Software pipeline: the global loads of a tile are issued into registers (fetch) BEFORE the tile in front of it is
// compressed and land in LDS after it (commit), so a wave's HBM latency hides under ~LPR/4 x 1.4k VALU of compression.
template <int T>
struct ShaTile {
  static_assert(T % 64 == 0 && T >= 64 && T <= 1024, "tile must be whole SHA blocks");
  static constexpr int ROW = T + 16;            // bytes
  static constexpr int LPR = T / 16;            // lanes that cover one row's tile
  static constexpr int RPI = 64 / LPR;          // rows per load instruction
  static constexpr size_t BYTES = 64 * ROW + 64 * 16;
  uint8_t* slab;
  uint8_t* desc;                                // 64 x {src(8), len(4), nblk(4)}
  uint8_t* my_row;                              // the lane's own message
  int lane;
  uint32_t my_len, my_nblk;
  uint4 stage[LPR];
  uint32_t live = 0;                            // bit g: stage[g] holds a row chunk that must be written to LDS

  __device__ __forceinline__ ShaTile(uint8_t* slab_, int lane_, const ShaLaneJob& J)
      : slab(slab_), desc(slab_ + 64 * ROW), my_row(slab_ + lane_ * ROW), lane(lane_), my_len(J.len), my_nblk(J.nblk) {}

  // the lane's descriptor row (by the wave that fetches)
  __device__ __forceinline__ void describe(const ShaLaneJob& J) {
    *(uint64_t*)(desc + lane * 16) = J.src;
    *(uint32_t*)(desc + lane * 16 + 8) = J.len;
    *(uint32_t*)(desc + lane * 16 + 12) = J.nblk;
  }
  __device__ __forceinline__ void fetch(uint32_t blk0) {
    const uint32_t tile_off = blk0 * 64;
    live = 0;
    uint4 dsc[LPR];                              // every row descriptor first (one ds_read_b128 each), then the loads
#pragma unroll
    for (int g = 0; g < LPR; g++) dsc[g] = *(const uint4*)(desc + (g * RPI + lane / LPR) * 16);
#pragma unroll
    for (int g = 0; g < LPR; g++) {
      const int chunk = lane % LPR;
      const uint64_t rsrc = ((uint64_t)dsc[g].y << 32) | dsc[g].x;
      const uint32_t rlen = dsc[g].z;
      const uint32_t rnblk = dsc[g].w;
      const uint32_t off = tile_off + chunk * 16;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (blk0 < rnblk) {                      // rows that are already finished are skipped
        live |= 1u << g;
        if (off + 16 <= rlen) {
          { const u32x4_raw t4 = *(gptr_u4)(rsrc + off); v = make_uint4(t4.x, t4.y, t4.z, t4.w); }
        } else if (off < rlen) {               // last partial chunk of the message: byte loads, never past the end
          gptr_u8 p = (gptr_u8)(rsrc + off);
          uint32_t rem = rlen - off, t[4] = {0, 0, 0, 0};
          for (uint32_t b = 0; b < rem; b++) t[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
          v = make_uint4(t[0], t[1], t[2], t[3]);
        }
      }
      stage[g] = v;
    }
  }
  __device__ __forceinline__ void commit(uint32_t blk0) {           // registers -> LDS slab, then the padding of this tile
    const uint32_t tile_off = blk0 * 64;
#pragma unroll
    for (int g = 0; g < LPR; g++) {
      const int row = g * RPI + lane / LPR;
      const int chunk = lane % LPR;
      if (live & (1u << g)) *(uint4*)(slab + row * ROW + chunk * 16) = stage[g];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- padding, patched into the lane's own row (FIPS 180-4 §5.1.1)
    if (blk0 < my_nblk) {
      if (my_len >= tile_off && my_len < tile_off + T) my_row[my_len - tile_off] = 0x80;
      const uint32_t last = my_nblk - 1;
      if (last >= blk0 && last < blk0 + T / 64) {
        const uint64_t bits = (uint64_t)my_len * 8;
        uint32_t* tail = (uint32_t*)(my_row + (last - blk0) * 64 + 56);
        tail[0] = __builtin_bswap32((uint32_t)(bits >> 32));
        tail[1] = __builtin_bswap32((uint32_t)bits);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

// The one-wave routine: every lane compresses its own message, a tile at a time; the next tile's loads are in flight
// during the compression.  sha1: this lane's message is a SHA-1 job.
template <int T>
__device__ __forceinline__ void sha_one_wave_tiles(ShaTile<T>& tile, uint32_t (&st)[8], uint32_t max_nblk, bool sha1) {
  if (max_nblk) { tile.fetch(0); tile.commit(0); }
  for (uint32_t blk0 = 0; blk0 < max_nblk; blk0 += T / 64) {
    const uint32_t next = blk0 + T / 64;
    const bool more = next < max_nblk;
    if (more) tile.fetch(next);                // in flight during the compression below
    // ---- compress: one message per lane
#pragma unroll 1
    for (int b = 0; b < T / 64; b++) {
      if (blk0 + b < tile.my_nblk) {
        uint32_t w[16];
        sha_load_block(w, tile.my_row + b * 64);
        if (sha1) sha1_compress(st, w); else sha256_compress(st, w);
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (more) tile.commit(next);
  }
}

// Launch: blockDim = 256 (4 independent waves), grid = ceil(n / 256).
// LDS (sha256_lds_bytes): 4 waves * (64 rows * (T + 16) bytes + 64 descriptors * 16 bytes) — 40 960 B per block at the
// engine's T = SHA_TILE = 128 (engine.hip); 73 728 B at T = 256.
template <int T>
__global__ __launch_bounds__(256) void sha256_batch_kernel(const ShaJob* __restrict__ jobs, uint32_t n) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  __builtin_amdgcn_s_setprio(ZKE_SHA_PRIO);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const uint32_t m = (blockIdx.x * 4 + wave) * 64 + lane;
  const ShaLaneJob J(jobs, m, n);
  ShaTile<T> tile(lds_raw + (size_t)wave * ShaTile<T>::BYTES, lane, J);
  tile.describe(J);
  const uint32_t max_nblk = J.wave_max_nblk();

  uint32_t st[8];
  const bool any_sha1 = J.wave_any_sha1();
  sha_init_state(st, J.algo != 0);
  sha_one_wave_tiles<T>(tile, st, max_nblk, any_sha1 && J.algo);
  if (m < n && J.dst) sha_store_digest((gptr_out32)J.dst, st, J.algo != 0);
}

template <int T>
constexpr size_t sha256_lds_bytes() { return 4 * (64 * (T + 16) + 64 * 16); }

// ---------------------------------------------------------------------------------------------------------------
// Two waves per 64 messages, for launches with few messages (the BASELINE batch: 1 024 bodies = 16 groups on a
// chip with 1 024 SIMDs).  Such a launch lasts as long as ONE wave needs for the longest message's chain of
// compressions, and a lone wave issues one instruction every ~4.3 cycles however independent its instructions
// are — so the only way to shorten the chain is to put fewer instructions on it.  The message schedule
// (W[16..63], ~480 VALU per block) does not depend on the chaining state: wave 0 (feeder) fetches the bytes,
// builds K[t] + W[t] for block k+1 and leaves the 64 words per lane in LDS while wave 1 (rounds) runs the 64
// rounds of block k from registers it filled from that buffer.  Two s_barriers per block; ~900 instead of ~1 400
// instructions on the critical path.  Groups that contain a SHA-1 job fall back to the one-wave routine.
// LDS per group: slab 64 x (T+16) + descriptors 1 KB + 64 lanes x 68 words of K+W (row stride 68 words = 4 banks
// mod 64: conflict-free 16-byte writes and reads, a quarter of the LDS instructions of word accesses).
constexpr int SHA_KW_ROW = 68;        // dwords per lane and buffer

template <int T>
constexpr size_t sha256_pair_lds_bytes() { return 64 * (T + 16) + 64 * 16 + 64 * SHA_KW_ROW * 4 + 1024; }      // slab, descriptors, K+W, job pick

// The job of each of a group's `width` positions (64, or 32 for sha256_twin_group) under length buckets (see ShaOrder): lane
// l < width of group g takes the message at global position width g + l of the longest-first order.  `pick`: 1 KB of LDS (192 class bases + 64 picks), written and read by the
// calling wave only.  Returns the lane's job index within the kind (SHA_KEY_NONE: no message), or `direct` when the batch is
// uniform enough for the direct mapping.  *skip = the whole group has nothing to do.
__device__ __forceinline__ uint32_t sha_pick_job(const ShaOrder& O, uint32_t g, uint32_t direct, uint32_t* pick, bool& skip, uint32_t width = 64) {
  const uint32_t lane = threadIdx.x & 63;
  skip = false;
  // class bases, longest class first: base[c] = messages in classes above c
  uint32_t c3[3], tot3 = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) { c3[k] = O.cnt[3 * lane + k]; tot3 += c3[k]; }
  const uint64_t nonempty = __ballot(tot3 != 0);
  if (!nonempty) { skip = true; return SHA_KEY_NONE; }
  {
    // uniform enough?  the non-empty classes span at most two neighbouring ones
    const uint32_t lo_lane = (uint32_t)__builtin_ctzll(nonempty), hi_lane = 63u - (uint32_t)__builtin_clzll(nonempty);
    uint32_t lo_c = 0xFFFFFFFFu, hi_c = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) if (c3[k]) { lo_c = min(lo_c, 3 * lane + k); hi_c = max(hi_c, 3 * lane + k); }
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)lo_c, (int)lo_lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)hi_c, (int)hi_lane);
    if (hi - lo <= 1) return direct;
  }
  uint32_t above = tot3;                                   // inclusive suffix sum over the lanes: messages in this lane's classes and above
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_down((int)above, o); if (lane + o < 64) above += t; }
  const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)above);
  if (width * g >= total) { skip = true; return SHA_KEY_NONE; }
  uint32_t b = above - tot3;                               // messages in the classes above this lane's
  pick[3 * lane + 2] = b; b += c3[2];
  pick[3 * lane + 1] = b; b += c3[1];
  pick[3 * lane + 0] = b;
  pick[SHA_CLASSES + lane] = SHA_KEY_NONE;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint32_t lo = width * g;
  for (uint32_t t0 = 0; t0 < O.n; t0 += 256) {             // four keys per lane and step: the loads of a step are in flight together
    uint32_t k4[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { const uint32_t i = t0 + 64 * q + lane; k4[q] = i < O.n ? O.key[i] : SHA_KEY_NONE; }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (k4[q] != SHA_KEY_NONE) {
        const uint32_t gp = pick[k4[q] >> 24] + (k4[q] & 0xFFFFFFu) - lo;
        if (gp < width) pick[SHA_CLASSES + gp] = t0 + 64 * q + lane;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return pick[SHA_CLASSES + lane];
}

// Length buckets in a two-wave group: the feeder (role 0) works the picks out, the rounds wave reads them.  Every thread of
// the group calls this (it uses __syncthreads()).  `order` nullptr or without counters: direct mapping, m stays.  Otherwise m
// becomes the lane's job under the buckets; true: the group has nothing to do and leaves as a whole.  A group of `width` < 64
// messages: `pos` is the thread's position in the group (its message is that of feeder lane pos; sha256_twin_group).
__device__ __forceinline__ bool sha_group_pick(const ShaOrder* order, uint32_t group, uint32_t& m, uint32_t* pick, int role,
                                               uint32_t width = 64, int pos = -1) {
  if (!(order && order->cnt)) return false;
  const int lane = threadIdx.x & 63;
  if (pos < 0) pos = lane;
  bool skip = false;
  uint32_t mine = 0;
  if (role == 0) {
    mine = sha_pick_job(*order, group, m, pick, skip, width);
    if (lane == 0) pick[SHA_CLASSES - 1] = skip ? 1u : 0u;          // (class 191 = 2^25 blocks and more: never populated)
    pick[SHA_CLASSES + lane] = mine;
  }
  __syncthreads();
  if (pick[SHA_CLASSES - 1]) return true;
  m = pick[SHA_CLASSES + pos];
  __syncthreads();                               // the pick area is dead from here (nobody writes it again)
  return false;
}

// Feeder: K[t] + W[t], t = 0..63, of the 64-byte block at `block` into kw_row (the lane's SHA_KW_ROW dwords of a K+W
// buffer: 16 ds_write_b128).
__device__ __forceinline__ void sha_kw_schedule(const uint8_t* block, uint32_t* kw_row) {
  uint32_t w[16];
  sha_load_block(w, block);
  uint4* dst = (uint4*)kw_row;
  uint32_t o4[4];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    uint32_t wi;
    if (i < 16) {
      wi = w[i];
    } else {
      const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
      const uint32_t s0 = xor3(rotr32(w15, 7), rotr32(w15, 18), w15 >> 3);
      const uint32_t s1 = xor3(rotr32(w2, 17), rotr32(w2, 19), w2 >> 10);
      wi = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
      w[i & 15] = wi;
    }
    o4[i & 3] = wi + SHA_K[i];
    if ((i & 3) == 3) dst[i >> 2] = make_uint4(o4[0], o4[1], o4[2], o4[3]);
  }
}

// Rounds wave: the 64 rounds of one block out of its K+W words in registers.  live: the lane's message has this block
// (the wave runs as many blocks as its longest message).
__device__ __forceinline__ void sha_rounds_kw(uint32_t (&st)[8], const uint4 (&kq)[16], bool live) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    const uint32_t S1 = xor3(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25));
    const uint4 k4 = kq[i >> 2];
    const uint32_t kwi = (i & 3) == 0 ? k4.x : (i & 3) == 1 ? k4.y : (i & 3) == 2 ? k4.z : k4.w;
    const uint32_t t1 = (h + S1 + ch3(e, f, g)) + kwi;
    const uint32_t S0 = xor3(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22));
    const uint32_t mj = maj3(a, b, c);
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
  }
  if (live) { st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h; }
}

// Dev knob (tests/cpp/sha_probe.hip, tools/sha_timeline.py): with ZKE_SHA_PROBE defined every wave of a two-role routine leaves
// its HW_ID register (SIMD, CU, ...) and XCC id, and the waves of group 0 a clock stamp at each marked point of blocks 8..15, in
// plain device arrays (ordinary vector stores).  The stamp's asm takes a chaining register in and out, so that the arithmetic in
// front of it and behind it stays there.  Without the define the product kernels carry none of it.
#ifdef ZKE_SHA_PROBE
constexpr uint32_t SHA_PROBE_GROUPS = 1024, SHA_PROBE_BLK0 = 8, SHA_PROBE_BLKS = 8, SHA_PROBE_SLOTS = 8;
__device__ uint32_t zke_sha_probe_hwid[SHA_PROBE_GROUPS][2][2];                              // [group][role]{HW_ID, XCC_ID}
__device__ unsigned long long zke_sha_probe_stamp[2][SHA_PROBE_BLKS][SHA_PROBE_SLOTS];       // [role][block - 8][point]
#define ZKE_SHA_WHERE() do { \
    if ((threadIdx.x & 63) == 0 && group < SHA_PROBE_GROUPS) { \
      zke_sha_probe_hwid[group][role][0] = __builtin_amdgcn_s_getreg(4 | (31 << 11)); \
      zke_sha_probe_hwid[group][role][1] = __builtin_amdgcn_s_getreg(20 | (31 << 11)); } } while (0)
#define ZKE_SHA_STAMP(kb, slot) do { \
    unsigned long long t_; \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_), "+v"(st[0]) : : "memory"); \
    if (group == 0 && (threadIdx.x & 63) == 0 && (kb) >= SHA_PROBE_BLK0 && (kb) < SHA_PROBE_BLK0 + SHA_PROBE_BLKS) \
      zke_sha_probe_stamp[role][(kb) - SHA_PROBE_BLK0][slot] = t_; } while (0)
#else
#define ZKE_SHA_WHERE() ((void)0)
#define ZKE_SHA_STAMP(kb, slot) ((void)0)
#endif

// The two waves of workgroup-local threads 0..127 hash messages [64 group, 64 group + 64); lds_raw: sha256_pair_lds_bytes<T>()
// of 16-byte aligned LDS.  A device routine so that other work can share the launch (fused.hip.h); both waves of the
// workgroup must call it (it uses __syncthreads()).
// `order`: length buckets of the jobs [0, n) this call sees (then `jobs` / `n` / `group` are the kind's), or nullptr.
template <int T>
__device__ __forceinline__ void sha256_pair_group(const ShaJob* __restrict__ jobs, uint32_t n, uint32_t group, uint8_t* lds_raw,
                                                  const ShaOrder* order = nullptr) {
  __builtin_amdgcn_s_setprio(ZKE_SHA_PRIO);
  const int lane = threadIdx.x & 63;
  const int role = threadIdx.x >> 6;               // 0 feeder, 1 rounds
  uint32_t* kw = (uint32_t*)(lds_raw + ShaTile<T>::BYTES);      // [64 lanes][SHA_KW_ROW]: a lane's 64 words are contiguous (b128 accesses)
  uint32_t* pick = kw + 64 * SHA_KW_ROW;           // 1 KB: sha_pick_job

  uint32_t m = group * 64 + lane;                  // both waves look at the same 64 jobs
  if (sha_group_pick(order, group, m, pick, role)) return;
  const ShaLaneJob J(jobs, m, n);
  const uint32_t max_nblk = J.wave_max_nblk();
  const bool any_sha1 = J.wave_any_sha1();         // the same in both waves: they read the same jobs

  uint32_t st[8];
  sha_init_state(st, false);
  ShaTile<T> tile(lds_raw, lane, J);
  if (role == 0) tile.describe(J);

  if (any_sha1) {
    // one-wave routine (as sha256_batch_kernel) by the feeder; the other wave has nothing to do.  No barrier below.
    if (role != 0) return;
    sha_init_state(st, J.algo != 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    sha_one_wave_tiles<T>(tile, st, max_nblk, J.algo != 0);
  } else {
    // feeder: K+W of block kb into the one buffer
    auto sched = [&](uint32_t kb) { sha_kw_schedule(tile.my_row + (kb % (T / 64)) * 64, kw + lane * SHA_KW_ROW); };
    if (role == 0 && max_nblk) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      tile.fetch(0); tile.commit(0);
      if (T / 64 < max_nblk) tile.fetch(T / 64);
      sched(0);
    }
    __syncthreads();
    // Both waves run exactly max_nblk steps (same jobs, same maximum).  ONE K+W buffer (a group then needs 28 KB of
    // LDS instead of 45 KB and finds room on a CU that front-end waves of other batches have nearly filled): the
    // rounds wave pulls the block's 64 words into registers, barrier, then the feeder overwrites the buffer with the
    // next block's while the rounds run from registers, barrier.
    ZKE_SHA_WHERE();
    for (uint32_t kb = 0; kb < max_nblk; kb++) {
      uint4 kq[16];
      ZKE_SHA_STAMP(kb, 0);
      if (role == 1) {
        const uint4* src = (const uint4*)(kw + lane * SHA_KW_ROW);
#pragma unroll
        for (int q = 0; q < 16; q++) kq[q] = src[q];
      }
      ZKE_SHA_STAMP(kb, 1);
      __syncthreads();                                // the buffer has been read
      ZKE_SHA_STAMP(kb, 2);
      if (role == 0) {
        const uint32_t nb = kb + 1;
        if (nb < max_nblk) {
          if (nb % (T / 64) == 0) {                  // first block of the next tile: its bytes were fetched a tile ago
            tile.commit(nb);
            if (nb + T / 64 < max_nblk) tile.fetch(nb + T / 64);
          }
          sched(nb);
        }
      } else {
        sha_rounds_kw(st, kq, kb < J.nblk);
      }
      ZKE_SHA_STAMP(kb, 3);
      __syncthreads();                                // the next block's words are in the buffer
      ZKE_SHA_STAMP(kb, 4);
    }
    if (role == 0) return;
  }
  if (m < n && J.dst) sha_store_digest((gptr_out32)J.dst, st, J.algo != 0);
}

template <int T>
__global__ __launch_bounds__(128) void sha256_pair_kernel(const ShaJob* __restrict__ jobs, uint32_t n) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  sha256_pair_group<T>(jobs, n, blockIdx.x, lds_raw);
}

// ---------------------------------------------------------------------------------------------------------------
// The ring: the same two roles, TWO K+W buffers and ONE barrier per block.  In the pair loop the rounds wave pulls the
// block's 64 words into registers in front of round 0 (16 ds_read_b128, a full lgkmcnt(0) drain, a barrier), and the feeder
// may not touch the buffer before that: the hand-over sits on the chain, and in the first block of every tile the feeder's commit
// + fetch + schedule is longer than the rounds, which then wait for it (profiles/sha_ring_timeline.txt: blocks of 4 700 and 5 840
// ticks for 3 970 ticks of rounds).
// Here the feeder writes block k + 1 into buffer (k + 1) & 1 while the rounds wave reads block k out of buffer k & 1 with no
// barrier between its reads and its rounds: the 16 reads go out together and round 4 q waits for quad q alone, so only the first
// quad's latency is in front of round 0.  45 KB of LDS per group instead of 28 KB, so it is the choice where few batches are on
// the chip (engine.hip).  Groups with a SHA-1 job go to sha256_pair_group (its one-wave path); so does nothing else.

template <int T>
constexpr size_t sha256_ring_lds_bytes() { return sha256_pair_lds_bytes<T>() + 64 * SHA_KW_ROW * 4; }   // slab, descriptors, K+W x 2, job pick

template <int T>
__device__ __forceinline__ void sha256_ring_group(const ShaJob* __restrict__ jobs, uint32_t n, uint32_t group, uint8_t* lds_raw,
                                                  const ShaOrder* order = nullptr) {
  constexpr int KW_BUF = 64 * SHA_KW_ROW;          // dwords per buffer
  __builtin_amdgcn_s_setprio(ZKE_SHA_PRIO);
  const int lane = threadIdx.x & 63;
  const int role = threadIdx.x >> 6;               // 0 feeder, 1 rounds
  uint32_t* kw = (uint32_t*)(lds_raw + ShaTile<T>::BYTES);      // [2 buffers][64 lanes][SHA_KW_ROW]
  uint32_t* pick = kw + 2 * KW_BUF;                // 1 KB: sha_pick_job

  uint32_t m = group * 64 + lane;
  if (sha_group_pick(order, group, m, pick, role)) return;
  const ShaLaneJob J(jobs, m, n);
  if (J.wave_any_sha1()) {                         // the same in both waves (same jobs): the pair routine's one-wave path.  It works the
    sha256_pair_group<T>(jobs, n, group, lds_raw, order);      // picks out again (rsa-sha1 is rare) in its own, smaller layout of this LDS
    return;
  }
  const uint32_t max_nblk = J.wave_max_nblk();

  uint32_t st[8];
  sha_init_state(st, false);
  ShaTile<T> tile(lds_raw, lane, J);
  if (role == 0) tile.describe(J);
  // feeder: K+W of block kb into buffer kb & 1
  auto sched = [&](uint32_t kb) { sha_kw_schedule(tile.my_row + (kb % (T / 64)) * 64, kw + (kb & 1) * KW_BUF + lane * SHA_KW_ROW); };
  // The block barrier: an s_barrier between LDS-only fences.  (__syncthreads() would also wait for the feeder's global
  // fetches of the next tile, which only commit() needs.)
  auto block_barrier = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  };
  if (role == 0 && max_nblk) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    tile.fetch(0); tile.commit(0);
    if (T / 64 < max_nblk) tile.fetch(T / 64);
    sched(0);
    if (T / 64 == 1 && 1 < max_nblk) tile.commit(1);
  }
  ZKE_SHA_WHERE();
  block_barrier();                                  // barrier -1: block 0's words are in buffer 0
  // Both waves run exactly max_nblk steps and one barrier per step.  In step kb the rounds wave reads buffer kb & 1 and the
  // feeder writes buffer (kb + 1) & 1.  That buffer was last read in step kb - 1, and every one of those reads had returned
  // (the rounds that use them were done) before the rounds wave arrived at barrier kb - 1, the one in front of this step: a
  // buffer is written only while no read of it is outstanding.  Barrier kb in turn puts the feeder's stores of step kb (its
  // release fence waits for them) in front of the reads of step kb + 1.
  for (uint32_t kb = 0; kb < max_nblk; kb++) {
    ZKE_SHA_STAMP(kb, 0);
    if (role == 0) {
      // The feeder's tile work is spread over the tile's steps, so that no step of it is longer than the rounds (in the pair
      // loop the first block of a tile carries commit + fetch + schedule, 5 100 cycles against the rounds' 3 900, and the
      // rounds wave waits for it at every second barrier): the next tile's loads go out in front of the tile's first
      // schedule, when the stage registers have just been emptied, and land in the slab behind its last schedule, when
      // the slab's bytes have all been read — the loads still have a whole tile's steps to arrive.
      const uint32_t nb = kb + 1;
      if (nb < max_nblk) {
        if (nb % (T / 64) == 0 && nb + T / 64 < max_nblk) tile.fetch(nb + T / 64);
        sched(nb);
        if (nb % (T / 64) == T / 64 - 1 && nb + 1 < max_nblk) tile.commit(nb + 1);
      }
    } else {
      const uint4* src = (const uint4*)(kw + (kb & 1) * KW_BUF + lane * SHA_KW_ROW);
      uint4 kq[16];                                 // all 16 reads go out here; each round group waits for its own quad only (lgkmcnt(N))
#pragma unroll
      for (int q = 0; q < 16; q++) kq[q] = src[q];
      // sha_rounds_kw written out: through the call all 16 reads stand in front of round 0, which waits for 13 of them: headline - 1.9 % (profiles/sha_shared_bench_ab.txt)
      uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
      for (int i = 0; i < 64; i++) {
        const uint32_t S1 = xor3(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25));
        const uint4 k4 = kq[i >> 2];
        const uint32_t kwi = (i & 3) == 0 ? k4.x : (i & 3) == 1 ? k4.y : (i & 3) == 2 ? k4.z : k4.w;
        const uint32_t t1 = (h + S1 + ch3(e, f, g)) + kwi;
        const uint32_t S0 = xor3(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22));
        const uint32_t mj = maj3(a, b, c);
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
      }
      if (kb < J.nblk) { st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h; }
    }
    ZKE_SHA_STAMP(kb, 1);
    block_barrier();                                // barrier kb
    ZKE_SHA_STAMP(kb, 2);
  }
  if (role == 0) return;
  if (m < n && J.dst) sha_store_digest((gptr_out32)J.dst, st, false);      // no SHA-1 job in a ring group
}

template <int T>
__global__ __launch_bounds__(128) void sha256_ring_kernel(const ShaJob* __restrict__ jobs, uint32_t n) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  sha256_ring_group<T>(jobs, n, blockIdx.x, lds_raw);
}

// ---------------------------------------------------------------------------------------------------------------
// The twin: the ring with a group of 32 messages and TWO LANES PER MESSAGE in the rounds wave.  What bounds a ring block is the
// rounds wave's own instruction count (14 VALU per round, one issue every ~4.8 cycles for a lone wave), and its lanes are free: so
// the two halves of a round go to two lanes.  The Σ functions are one instruction sequence with different rotation amounts
// (v_alignbit_b32 takes its amount from a VGPR), and Maj(a, b, c) = Ch(a ^ c, b, c), so lane A of a pair holds e, f, g, h, lane B
// holds a, b, c, d, in the same four registers R0..R3, and one round is
//   r1, r2, r3 = alignbit(R0, R0, sh0 | sh1 | sh2)   3   sh* per lane (SHA_TWIN_SH): A 6, 11, 25   B 2, 13, 22
//   S = bitop3(r1, r2, r3, 0x96)                     1   A: Σ1(e)              B: Σ0(a)
//   D = bitop3(R0, R2, maskb, 0x78)                  1   A: e                  B: a ^ c       (x ^ (z & m); maskb 0 on A, ~0 on B)
//   F = bitop3(D, R1, R2, 0xCA)                      1   A: Ch(e, f, g)        B: Maj(a, b, c)
//   U = add3(S, F, KW)                               1   A: Σ1 + Ch + K + W    B: Σ0 + Maj    (B lanes read zeros for K + W)
//   R3 = R3 + U      A lanes only                    1   A: t1                 B: d
//   U  = 0 | R3      A lanes only                    1   A: t1                 B: Σ0 + Maj
//   N  = R3[partner] + U                             1   A: d + t1 = e'        B: t1 + Σ0 + Maj = a'
//   R3 <- R2 <- R1 <- R0 <- N
// 10 VALU instead of 14, and the Davies-Meyer add is 4 instead of 8.  The last three are DPP instructions (sha_twin_exchange),
// and the third reads R3 through DPP two instructions behind its write: a wait state in every round, and a second one that the
// compiler puts behind every asm statement.  On a wave that is alone on its SIMD an s_nop costs the issue slot of a VALU
// instruction, so that is the round of the ZKE_SHA_TWIN_NOWAIT = 0 build only.  The default round hands t1 and d across the pair
// so that no DPP operand is read sooner than three instructions behind its write, with Q = h + K + W on A lanes and 0 on B lanes:
//   r1, r2, r3, S, D, F                              6   as above
//   W  = add3(S, F, Q)                               1   A: h + Σ1 + Ch + K + W = t1   B: Σ0 + Maj
//   N  = R3[partner] + W      all lanes              1   A: d + t1 = e'                B: (h + Σ0 + Maj: overwritten below)
//   Q' = Q' + R2              A lanes only           1   the next round's Q, in place in its K + W register: R2 is that round's R3
//   N  = W[partner] + W       B lanes only           1   B: t1 + Σ0 + Maj = a'
//   R3 <- R2 <- R1 <- R0 <- N
// W is the only register read through DPP soon after its write, and N and Q' stand between the two; R3 and R2 were written two
// and more rounds ago; K + W comes from LDS.  B lanes read zeros for K + W and the masked add does not write them: their Q stays
// 0.  N goes into the register of the dying R3, so after four rounds every value is in its own register again and a block is
// ONE asm statement of 16 quads (sha_twin_block_nowait) with no move in it; the compiler's wait state follows the statement,
// once per block.  Round 0's Q is made in front of its add3 (it reads R3 through DPP; the state was written by the block in
// front), round 63 has no next K + W and an s_nop 0 in the slot.
// Pairs: lane l and lane l ^ 7 (row_half_mirror: 7 - l within each eight); A lanes are those with (l & 4) == 0 (bank_mask 0x5 of an
// identity quad_perm), so message p of the group sits in lanes 8 (p / 4) + p % 4 (A) and 8 (p / 4) + 7 - p % 4 (B).
// The feeder wave's 64 lanes then serve two blocks of the 32 messages at once: lane l < 32 schedules block 2 j of message l, lane
// l + 32 block 2 j + 1 — with T = 128 exactly the two blocks of a slab row —, so one feeder pass (schedule, commit, fetch) serves
// two steps of the rounds wave, and there is one barrier per pass.  K+W row 32 h + p of buffer j & 1 is block 2 j + h of message p.
// Slab rows 32..63 hold no message (their descriptors say nblk 0); the first 256 bytes of row 32 are the zeros the B lanes read.
// LDS and workgroup shape are the ring's.  Groups with a SHA-1 job take the one-wave path, here, 32 wide.
// (SHA_TWIN_WIDTH, the messages per group: stage_plan.hip.h)
constexpr uint32_t SHA_TWIN_SH[2][3] = {{6, 11, 25}, {2, 13, 22}};      // [A | B]: Σ1, Σ0
constexpr uint32_t SHA_TWIN_MASKB[2] = {0u, 0xFFFFFFFFu};

// the lane's half of its pair, and its message's position in the group
__device__ __forceinline__ bool sha_twin_is_b(int lane) { return (lane & 4) != 0; }
__device__ __forceinline__ int sha_twin_pos(int lane) { return (lane >> 3) * 4 + (sha_twin_is_b(lane) ? 7 - (lane & 7) : (lane & 3)); }

// The three DPP steps of a round.  The masked add takes the old R3 as its DPP operand and the fresh U as its plain one; the masked
// OR takes R3 as its plain operand (the DPP one is a register of zeros): neither reads through DPP what the instruction in front
// wrote.  The last add reads R3 through DPP two instructions behind its write: one wait state (the rule of rsa.hip.h's dpp
// helpers; the compiler does not look inside an asm).  Callers keep a VALU write of r3 two wait states away from this asm.
__device__ __forceinline__ uint32_t sha_twin_exchange(uint32_t& r3, uint32_t u, uint32_t zero) {
  uint32_t n;
  asm("v_add_u32_dpp %1, %1, %2 quad_perm:[0,1,2,3] row_mask:0xf bank_mask:0x5\n\t"
      "v_or_b32_dpp %2, %3, %1 quad_perm:[0,1,2,3] row_mask:0xf bank_mask:0x5\n\t"
      "s_nop 0\n\t"
      "v_add_u32_dpp %0, %1, %2 row_half_mirror row_mask:0xf bank_mask:0xf"
      : "=&v"(n), "+v"(r3), "+v"(u)
      : "v"(zero));
  return n;
}

// ZKE_SHA_TWIN_NOWAIT (default 1): the round without wait states; 0 builds the round of sha_twin_exchange from the same source
// (tools/build_variant.sh).
#ifndef ZKE_SHA_TWIN_NOWAIT
#define ZKE_SHA_TWIN_NOWAIT 1
#endif

// One round of the default build as asm text.  R0..R3: the registers in this round's roles; KW: the round's Q; PRE stands in front
// of the add3 (round 0: its own Q), NEXT in the slot between N and the B lanes' N (the next round's Q, with the wait for its
// quad where it is a quad's first word).
#define ZKE_TW_Q(R, KW) "v_add_u32_dpp " KW ", " R ", " KW " quad_perm:[0,1,2,3] row_mask:0xf bank_mask:0x5\n\t"
#define ZKE_TW_ROUND(R0, R1, R2, R3, KW, PRE, NEXT) \
  "v_alignbit_b32 %[t0], " R0 ", " R0 ", %[sh0]\n\t" \
  "v_alignbit_b32 %[t1], " R0 ", " R0 ", %[sh1]\n\t" \
  "v_alignbit_b32 %[t2], " R0 ", " R0 ", %[sh2]\n\t" \
  "v_bitop3_b32 %[t0], %[t0], %[t1], %[t2] bitop3:0x96\n\t" \
  "v_bitop3_b32 %[t1], " R0 ", " R2 ", %[mb] bitop3:0x78\n\t" \
  "v_bitop3_b32 %[t1], %[t1], " R1 ", " R2 " bitop3:0xca\n\t" \
  PRE \
  "v_add3_u32 %[t0], %[t0], %[t1], " KW "\n\t" \
  "v_add_u32_dpp " R3 ", " R3 ", %[t0] row_half_mirror row_mask:0xf bank_mask:0xf\n\t" \
  NEXT \
  "v_add_u32_dpp " R3 ", %[t0], %[t0] row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
// Four rounds: the words of quad K0..K3, then NEXT3 (the first word of the quad behind it).  The roles rotate through the four
// state registers and are back where they were.
#define ZKE_TW_QUAD(K0, K1, K2, K3, PRE0, NEXT3) \
  ZKE_TW_ROUND("%[r0]", "%[r1]", "%[r2]", "%[r3]", K0, PRE0, ZKE_TW_Q("%[r2]", K1)) \
  ZKE_TW_ROUND("%[r3]", "%[r0]", "%[r1]", "%[r2]", K1, "", ZKE_TW_Q("%[r1]", K2)) \
  ZKE_TW_ROUND("%[r2]", "%[r3]", "%[r0]", "%[r1]", K2, "", ZKE_TW_Q("%[r0]", K3)) \
  ZKE_TW_ROUND("%[r1]", "%[r2]", "%[r3]", "%[r0]", K3, "", NEXT3)
#define ZKE_TW_WAIT(N) "s_waitcnt lgkmcnt(" #N ")\n\t"
#define ZKE_TW_READ(V, OFF) "ds_read_b128 " V ", %[src] offset:" #OFF "\n\t"

// The 64 rounds of one block on r0..r3 (R0..R3), K + W from the 256 bytes at LDS address `src`.  The words go into v64..v127,
// which the statement names itself: as components of operands the compiler would copy three words of every quad in front of the
// statement, since the rounds add to them in place.  All 16 reads go out in front of round 0 and each quad is waited for alone, as
// in the ring: lgkmcnt counts to 15, so the first wait (14) is for quads 0 and 1 and quad q >= 2 has arrived at 15 - q.  The
// compiler does not see these counts, so the statement makes them its own with a wait in front of the reads: the wave's ds_write
// of the zeros in front of block 0, and whatever else of LDS or scalar memory the code in front left counted, is done by then.
// (Behind a block barrier its release fence has drained the counter already.)
__device__ __forceinline__ void sha_twin_block_nowait(uint32_t& r0, uint32_t& r1, uint32_t& r2, uint32_t& r3, uint32_t src,
                                                      uint32_t sh0, uint32_t sh1, uint32_t sh2, uint32_t maskb) {
  uint32_t t0, t1, t2;
  asm volatile(
      "s_waitcnt lgkmcnt(0)\n\t"
      ZKE_TW_READ("v[64:67]", 0) ZKE_TW_READ("v[68:71]", 16) ZKE_TW_READ("v[72:75]", 32) ZKE_TW_READ("v[76:79]", 48)
      ZKE_TW_READ("v[80:83]", 64) ZKE_TW_READ("v[84:87]", 80) ZKE_TW_READ("v[88:91]", 96) ZKE_TW_READ("v[92:95]", 112)
      ZKE_TW_READ("v[96:99]", 128) ZKE_TW_READ("v[100:103]", 144) ZKE_TW_READ("v[104:107]", 160) ZKE_TW_READ("v[108:111]", 176)
      ZKE_TW_READ("v[112:115]", 192) ZKE_TW_READ("v[116:119]", 208) ZKE_TW_READ("v[120:123]", 224) ZKE_TW_READ("v[124:127]", 240)
      ZKE_TW_QUAD("v64", "v65", "v66", "v67", ZKE_TW_WAIT(14) ZKE_TW_Q("%[r3]", "v64"), ZKE_TW_Q("%[r3]", "v68"))
      ZKE_TW_QUAD("v68", "v69", "v70", "v71", "", ZKE_TW_WAIT(13) ZKE_TW_Q("%[r3]", "v72"))
      ZKE_TW_QUAD("v72", "v73", "v74", "v75", "", ZKE_TW_WAIT(12) ZKE_TW_Q("%[r3]", "v76"))
      ZKE_TW_QUAD("v76", "v77", "v78", "v79", "", ZKE_TW_WAIT(11) ZKE_TW_Q("%[r3]", "v80"))
      ZKE_TW_QUAD("v80", "v81", "v82", "v83", "", ZKE_TW_WAIT(10) ZKE_TW_Q("%[r3]", "v84"))
      ZKE_TW_QUAD("v84", "v85", "v86", "v87", "", ZKE_TW_WAIT(9) ZKE_TW_Q("%[r3]", "v88"))
      ZKE_TW_QUAD("v88", "v89", "v90", "v91", "", ZKE_TW_WAIT(8) ZKE_TW_Q("%[r3]", "v92"))
      ZKE_TW_QUAD("v92", "v93", "v94", "v95", "", ZKE_TW_WAIT(7) ZKE_TW_Q("%[r3]", "v96"))
      ZKE_TW_QUAD("v96", "v97", "v98", "v99", "", ZKE_TW_WAIT(6) ZKE_TW_Q("%[r3]", "v100"))
      ZKE_TW_QUAD("v100", "v101", "v102", "v103", "", ZKE_TW_WAIT(5) ZKE_TW_Q("%[r3]", "v104"))
      ZKE_TW_QUAD("v104", "v105", "v106", "v107", "", ZKE_TW_WAIT(4) ZKE_TW_Q("%[r3]", "v108"))
      ZKE_TW_QUAD("v108", "v109", "v110", "v111", "", ZKE_TW_WAIT(3) ZKE_TW_Q("%[r3]", "v112"))
      ZKE_TW_QUAD("v112", "v113", "v114", "v115", "", ZKE_TW_WAIT(2) ZKE_TW_Q("%[r3]", "v116"))
      ZKE_TW_QUAD("v116", "v117", "v118", "v119", "", ZKE_TW_WAIT(1) ZKE_TW_Q("%[r3]", "v120"))
      ZKE_TW_QUAD("v120", "v121", "v122", "v123", "", ZKE_TW_WAIT(0) ZKE_TW_Q("%[r3]", "v124"))
      ZKE_TW_QUAD("v124", "v125", "v126", "v127", "", "s_nop 0\n\t")
      : [r0] "+v"(r0), [r1] "+v"(r1), [r2] "+v"(r2), [r3] "+v"(r3), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2)
      : [src] "v"(src), [sh0] "v"(sh0), [sh1] "v"(sh1), [sh2] "v"(sh2), [mb] "v"(maskb)
      : "memory", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79",
        "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95",
        "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111",
        "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
}
#undef ZKE_TW_READ
#undef ZKE_TW_WAIT
#undef ZKE_TW_QUAD
#undef ZKE_TW_ROUND
#undef ZKE_TW_Q

template <int T>
__device__ __forceinline__ void sha256_twin_group(const ShaJob* __restrict__ jobs, uint32_t n, uint32_t group, uint8_t* lds_raw,
                                                  const ShaOrder* order = nullptr) {
  static_assert(T == 128, "a slab row is the two blocks of a feeder pass");
  constexpr int KW_BUF = 64 * SHA_KW_ROW;          // dwords per buffer
  constexpr int ROW = ShaTile<T>::ROW;
  __builtin_amdgcn_s_setprio(ZKE_SHA_PRIO);
  const int lane = threadIdx.x & 63;
  const int role = threadIdx.x >> 6;               // 0 feeder, 1 rounds
  uint32_t* kw = (uint32_t*)(lds_raw + ShaTile<T>::BYTES);      // [2 buffers][2 block parities][32 messages][SHA_KW_ROW]
  uint32_t* pick = kw + 2 * KW_BUF;                // 1 KB: sha_pick_job
  uint8_t* zeros = lds_raw + 32 * ROW;             // 256 bytes in the slab's unused rows

  const bool is_b = sha_twin_is_b(lane);
  const int pos = role == 0 ? (lane & 31) : sha_twin_pos(lane);      // the message: two feeder lanes and a rounds pair each
  const int half = lane >> 5;                      // feeder: which block of the pass
  uint32_t m = group * SHA_TWIN_WIDTH + pos;
  if (sha_group_pick(order, group, m, pick, role, SHA_TWIN_WIDTH, pos)) return;
  const ShaLaneJob J(jobs, m, n);
  const ShaLaneJob none(jobs, n, n);
  const uint32_t max_nblk = J.wave_max_nblk();     // the same in both waves: each sees the 32 jobs twice

  if (J.wave_any_sha1()) {
    // one-wave routine by the feeder's lower lanes, a message each; no barrier below
    if (role != 0) return;
    const ShaLaneJob J1 = half ? none : J;
    uint32_t st[8];
    sha_init_state(st, J1.algo != 0);
    ShaTile<T> tile(lds_raw, lane, J1);
    tile.describe(J1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    sha_one_wave_tiles<T>(tile, st, max_nblk, J1.algo != 0);
    if (!half && m < n && J1.dst) sha_store_digest((gptr_out32)J1.dst, st, J1.algo != 0);
    return;
  }

  const uint32_t passes = (max_nblk + 1) / 2;
  // The block barrier: an s_barrier between LDS-only fences, as in the ring.
  auto block_barrier = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  };
  // In pass j the rounds wave reads buffer j & 1 (steps 2 j and 2 j + 1) and the feeder writes buffer (j + 1) & 1; barrier j - 1
  // stands behind the last read of that buffer and barrier j in front of the first read of what the feeder wrote: the ring's
  // argument with a pass for a step.  Both waves run `passes` barriers behind barrier -1.
  if (role == 0) {
    // ---- feeder.  Rows 32..63 are described as empty, and the upper lanes patch no padding: the lower lane of a row does.
    ShaTile<T> tile(lds_raw, lane, J);
    tile.my_row = lds_raw + pos * ROW;
    if (half) tile.my_nblk = 0;
    tile.describe(half ? none : J);
    // K+W of block 2 j + half of message pos into row `lane` of buffer j & 1 (an odd max_nblk: the upper lanes idle in the last pass)
    auto sched = [&](uint32_t j) {
      if (2 * j + half < max_nblk) sha_kw_schedule(tile.my_row + half * 64, kw + (j & 1) * KW_BUF + lane * SHA_KW_ROW);
    };
    // a tile's loads go out behind the commit of the tile in front of it and land a whole pass later
    auto next_tile = [&](uint32_t j) {
      if (j < passes) { tile.commit(2 * j); if (j + 1 < passes) tile.fetch(2 * (j + 1)); }
    };
    if (passes) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      tile.fetch(0);
      next_tile(0);
      sched(0);
      next_tile(1);
    }
    ZKE_SHA_WHERE();
    block_barrier();                                // barrier -1: blocks 0 and 1 are in buffer 0
    uint32_t st[1] = {0};                           // (the probe's stamps thread a register through)
    for (uint32_t j = 0; j < passes; j++) {
      ZKE_SHA_STAMP(2 * j, 0);
      if (j + 1 < passes) { sched(j + 1); next_tile(j + 2); }
      ZKE_SHA_STAMP(2 * j, 1);
      block_barrier();                              // barrier j
      ZKE_SHA_STAMP(2 * j, 2);
    }
    (void)st;
    return;
  }

  // ---- rounds: st = the lane's half of the chaining state, e..h on A lanes and a..d on B lanes
  uint32_t st[4];
  {
    uint32_t iv[8];
    sha_init_state(iv, false);
#pragma unroll
    for (int i = 0; i < 4; i++) st[i] = is_b ? iv[i] : iv[4 + i];
  }
  const uint32_t sh0 = is_b ? SHA_TWIN_SH[1][0] : SHA_TWIN_SH[0][0], sh1 = is_b ? SHA_TWIN_SH[1][1] : SHA_TWIN_SH[0][1];
  const uint32_t sh2 = is_b ? SHA_TWIN_SH[1][2] : SHA_TWIN_SH[0][2], maskb = is_b ? SHA_TWIN_MASKB[1] : SHA_TWIN_MASKB[0];
#if !ZKE_SHA_TWIN_NOWAIT
  uint32_t zero = 0;
  asm volatile("" : "+v"(zero));                    // a register of its own, not a literal in the asm
#endif
  if (lane < 16) ((uint4*)zeros)[lane] = make_uint4(0, 0, 0, 0);
  ZKE_SHA_WHERE();
  block_barrier();                                  // barrier -1 (the zeros are this wave's own: in order behind its store)
  for (uint32_t kb = 0; kb < max_nblk; kb++) {
    ZKE_SHA_STAMP(kb, 0);
    const uint4* src = is_b ? (const uint4*)zeros
                            : (const uint4*)(kw + ((kb >> 1) & 1) * KW_BUF + ((kb & 1) * 32 + pos) * SHA_KW_ROW);
#if ZKE_SHA_TWIN_NOWAIT
    uint32_t r0 = st[0], r1 = st[1], r2 = st[2], r3 = st[3];
    sha_twin_block_nowait(r0, r1, r2, r3, (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint4*)src, sh0, sh1, sh2, maskb);
#else
    uint4 kq[16];                                   // all 16 reads go out here; each round group waits for its own quad only
#pragma unroll
    for (int q = 0; q < 16; q++) kq[q] = src[q];
    uint32_t r0 = st[0], r1 = st[1], r2 = st[2], r3 = st[3];
    asm volatile("s_nop 1" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));      // whatever wrote them is two wait states away from the first DPP read
    // the rounds written out, as in the ring and for its reason
#pragma unroll
    for (int i = 0; i < 64; i++) {
      const uint32_t s = xor3(__builtin_amdgcn_alignbit(r0, r0, sh0), __builtin_amdgcn_alignbit(r0, r0, sh1), __builtin_amdgcn_alignbit(r0, r0, sh2));
      const uint32_t d = __builtin_amdgcn_bitop3_b32(r0, r2, maskb, 0x78);
      const uint32_t f = ch3(d, r1, r2);
      const uint4 k4 = kq[i >> 2];
      const uint32_t kwi = (i & 3) == 0 ? k4.x : (i & 3) == 1 ? k4.y : (i & 3) == 2 ? k4.z : k4.w;
      const uint32_t u = s + f + kwi;
      const uint32_t nw = sha_twin_exchange(r3, u, zero);
      r3 = r2; r2 = r1; r1 = r0; r0 = nw;
    }
#endif
    if (kb < J.nblk) { st[0] += r0; st[1] += r1; st[2] += r2; st[3] += r3; }
    ZKE_SHA_STAMP(kb, 1);
    if ((kb & 1) || kb + 1 == max_nblk) block_barrier();       // barrier kb / 2: the pass is read
    ZKE_SHA_STAMP(kb, 2);
  }
  if (m < n && J.dst) {                             // a..d by the B lane, e..h by the A lane; no SHA-1 job in a twin group
    gptr_out32 out = (gptr_out32)J.dst + (is_b ? 0 : 4);
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = __builtin_bswap32(st[i]);
  }
}

// grid = ceil(n / 32)
template <int T>
__global__ __launch_bounds__(128) void sha256_twin_kernel(const ShaJob* __restrict__ jobs, uint32_t n) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  sha256_twin_group<T>(jobs, n, blockIdx.x, lds_raw);
}

}  // namespace zke
