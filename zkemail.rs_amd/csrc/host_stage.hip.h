// host_stage.hip.h — the host side of the host-memory entry point (zke_verify_batch[_async]): pinned staging memory and the
// worker threads that fill it.
//
// The drop-in caller holds `&[Email]` in ordinary (pageable) RAM (core/src/circuits.rs:9; built at
// helpers/src/generator.rs:40-45).  A DMA engine reads pinned memory only, so every byte crosses the host's memory once
// before it crosses PCIe: pageable -> the slot's pinned image (here, by `host_threads` threads: one thread copies ~10 GB/s,
// a Gen5 x16 link moves ~55), then ONE hipMemcpyAsync of the whole image on the slot's stream.  Included by engine.hip.
#pragma once

#include <condition_variable>
#include <functional>
#include <thread>
#include <immintrin.h>

namespace {

struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t need) {
    if (need <= cap) return 0;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const size_t want = std::max(need + need / 4, (size_t)4096);
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return ZKE_E_NOMEM; }
    cap = want;
    return 0;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
  void track(uint64_t*) {}             // (pinned memory is in no captured graph: DevBuf::track)
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// The shape of a side output's buffers (captures, scan, key records, bodies, origins): a device buffer the kernels write and a pinned
// twin of the same layout; a prefix of it comes back as ONE copy on the batch's stream.
struct TwinBuf {
  DevBuf d;
  PinnedBuf h;
  int ensure(size_t device_bytes, size_t pinned_bytes) { if (int r = d.ensure(device_bytes)) return r; return h.ensure(pinned_bytes); }
  void release() { d.release(); h.release(); }
  hipError_t fetch(size_t bytes, hipStream_t s) const { return hipMemcpyAsync(h.p, d.p, bytes, hipMemcpyDeviceToHost, s); }
};
// Every buffer a struct owns, once: f(DevBuf&) or f(PinnedBuf&).  One overload per struct, next to it; Slot::each_buffer walks them all.
template <class F> void each_buffer(DevBuf& b, F& f) { f(b); }
template <class F> void each_buffer(PinnedBuf& b, F& f) { f(b); }
template <class F> void each_buffer(TwinBuf& b, F& f) { f(b.d); f(b.h); }
// A building block's temporary: released on every way out of its scope.  (A slot's buffers live as long as the slot and stay plain.)
template <class B> struct Scoped : B {
  Scoped() = default;
  Scoped(const Scoped&) = delete; Scoped& operator=(const Scoped&) = delete;
  ~Scoped() { this->release(); }
};

// Pageable -> pinned, streaming: non-temporal stores.  An ordinary memcpy of a piece this size reads the destination lines
// before it overwrites them (read-for-ownership) and leaves the image in the cache hierarchy, where nobody will read it — the
// DMA engine reads memory.  Streaming stores move two bytes per byte copied instead of three.  dst is 32-byte aligned (pieces
// start on 64-byte boundaries of a 4 KiB-aligned pinned buffer); the head and tail go through memcpy.
__attribute__((target("avx2"))) inline void stream_copy_avx2(uint8_t* dst, const uint8_t* src, size_t n) {
  size_t head = (32 - ((uintptr_t)dst & 31)) & 31;
  if (head > n) head = n;
  if (head) { memcpy(dst, src, head); dst += head; src += head; n -= head; }
  size_t i = 0;
  for (; i + 128 <= n; i += 128) {
    const __m256i a = _mm256_loadu_si256((const __m256i*)(src + i)), b = _mm256_loadu_si256((const __m256i*)(src + i + 32)),
                  c = _mm256_loadu_si256((const __m256i*)(src + i + 64)), d = _mm256_loadu_si256((const __m256i*)(src + i + 96));
    _mm256_stream_si256((__m256i*)(dst + i), a); _mm256_stream_si256((__m256i*)(dst + i + 32), b);
    _mm256_stream_si256((__m256i*)(dst + i + 64), c); _mm256_stream_si256((__m256i*)(dst + i + 96), d);
  }
  _mm_sfence();
  if (i < n) memcpy(dst + i, src + i, n - i);
}
inline void stage_copy(void* dst, const void* src, size_t n, size_t stream_from = 64u << 10) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (!n) return;          // (an empty table may have no address at all: nothing for memcpy to be handed)
  if (avx2 && n >= stream_from) stream_copy_avx2((uint8_t*)dst, (const uint8_t*)src, n);
  else memcpy(dst, src, n);
}

// A handful of threads that do nothing but memcpy.  Several callers may use the pool at once (each call waits for its own
// pieces only); with one thread configured, or for small copies, the caller's thread does the work itself.
#ifndef ZKE_GATHER_STREAM_FROM
#define ZKE_GATHER_STREAM_FROM 1024
#endif
#ifndef ZKE_GATHER_VIA_BUFFER
#define ZKE_GATHER_VIA_BUFFER 1
#endif
#ifndef ZKE_GATHER_CHUNK
#define ZKE_GATHER_CHUNK (256u << 10)
#endif
class CopyPool {
 public:
  explicit CopyPool(unsigned workers) {
    for (unsigned i = 0; i < workers; i++) threads_.emplace_back([this] { run(); });
  }
  ~CopyPool() {
    { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }
  // the pieces of one packing job; returns when all of them are done
  struct Piece { void* dst; const void* src; size_t n; };
  void copy(const Piece* pieces, size_t count) {
    constexpr size_t CHUNK = 256 << 10;           // below this a hand-over costs more than the copy
    std::vector<Piece> work;
    for (size_t i = 0; i < count; i++) {
      const Piece& p = pieces[i];
      if (!p.n) continue;
      if (threads_.empty() || p.n < 2 * CHUNK) { work.push_back(p); continue; }
      // (one part per thread: 256 KB parts of a blob, as the gather has them, lose 5-10 % here — measured, tools/ab_scattered.sh)
      const size_t parts = std::min<size_t>(threads_.size() + 1, (p.n + CHUNK - 1) / CHUNK);
      const size_t step = ((p.n + parts - 1) / parts + 63) & ~(size_t)63;
      for (size_t o = 0; o < p.n; o += step)
        work.push_back(Piece{(uint8_t*)p.dst + o, (const uint8_t*)p.src + o, std::min(step, p.n - o)});
    }
    if (work.empty()) return;
    size_t big = 0;
    for (const Piece& p : work) big += p.n >= CHUNK;
    if (threads_.empty() || big < 2) {            // nothing worth sharing
      for (const Piece& p : work) stage_copy(p.dst, p.src, p.n);
      return;
    }
    std::vector<Task> tasks;
    tasks.reserve(work.size());
    for (const Piece& p : work) tasks.push_back(Task{&p, 1, 64u << 10, nullptr});
    run_job(tasks);
  }
  // Many small pieces whose destinations follow each other (the e-mails of a batch handed over one by one, each in its own
  // buffer: `&[Email]` as the reference holds it): consecutive pieces are grouped into tasks of ~256 KB, so a thread is handed a
  // run of e-mails, not one; pieces of a kilobyte and more go through streaming stores.
  void gather(const Piece* pieces, size_t count) {
    constexpr size_t CHUNK = 256 << 10;
    size_t total = 0;
    for (size_t i = 0; i < count; i++) total += pieces[i].n;
    if (threads_.empty() || total < 2 * CHUNK) {
      for (size_t i = 0; i < count; i++) if (pieces[i].n) stage_copy(pieces[i].dst, pieces[i].src, pieces[i].n, ZKE_GATHER_STREAM_FROM);
      return;
    }
    // A task is a run of pieces whose destinations follow each other without a gap, cut at ~256 KB: the thread that takes it
    // collects the run in a buffer of its own (the sources are scattered, the buffer stays in its cache) and writes it out as
    // ONE streaming copy — a streaming copy per 5 KB piece pays a fence and two partial lines (head, tail) per e-mail, and
    // mixes ordinary and write-combining stores on the lines where two e-mails meet.
    std::vector<Task> tasks;
    size_t first = 0, bytes = 0;
    for (size_t i = 0; i < count; i++) {
      bytes += pieces[i].n;
      const bool gap = i + 1 < count && (const uint8_t*)pieces[i + 1].dst != (const uint8_t*)pieces[i].dst + pieces[i].n;
      if (bytes >= ZKE_GATHER_CHUNK || gap || i + 1 == count) {
        tasks.push_back(Task{pieces + first, i + 1 - first, ZKE_GATHER_STREAM_FROM, nullptr, ZKE_GATHER_VIA_BUFFER != 0});
        first = i + 1; bytes = 0;
      }
    }
    run_job(tasks);
  }

 private:
  struct Job { std::mutex mu; std::condition_variable cv; size_t left = 0; };
  struct Task { const Piece* p; size_t cnt; size_t stream_from; Job* job; bool run = false; };   // run: the pieces' destinations are contiguous
  // hand the tasks to the pool, work along, return when all of them are done (`tasks` and what they point to outlive the call)
  void run_job(std::vector<Task>& tasks) {
    if (tasks.empty()) return;
    Job job;
    job.left = tasks.size();
    {
      std::lock_guard<std::mutex> g(mu_);
      for (Task& t : tasks) { t.job = &job; queue_.push_back(t); }
      pending_.fetch_add((int)tasks.size(), std::memory_order_release);
    }
    cv_.notify_all();
    // the caller works too: it takes tasks until the queue is empty, then waits for the stragglers
    for (;;) {
      Task t;
      {
        std::lock_guard<std::mutex> g(mu_);
        if (queue_.empty()) break;
        t = queue_.back(); queue_.pop_back(); pending_.fetch_sub(1, std::memory_order_relaxed);
      }
      do_task(t);
    }
    std::unique_lock<std::mutex> lk(job.mu);
    job.cv.wait(lk, [&] { return job.left == 0; });
  }
  void do_task(const Task& t) {
    if (t.run && t.cnt > 1) {
      static thread_local std::vector<uint8_t> buf;
      size_t total = 0;
      for (size_t i = 0; i < t.cnt; i++) total += t.p[i].n;
      if (buf.size() < total) buf.resize(total + (64u << 10));
      size_t o = 0;
      for (size_t i = 0; i < t.cnt; i++) if (t.p[i].n) { memcpy(buf.data() + o, t.p[i].src, t.p[i].n); o += t.p[i].n; }
      if (total) stage_copy(t.p[0].dst, buf.data(), total, t.stream_from);
    } else
    for (size_t i = 0; i < t.cnt; i++) if (t.p[i].n) stage_copy(t.p[i].dst, t.p[i].src, t.p[i].n, t.stream_from);
    std::lock_guard<std::mutex> g(t.job->mu);
    if (--t.job->left == 0) t.job->cv.notify_all();
  }
  void run() {
    for (;;) {
      Task t;
      bool have = false;
      // A streaming caller hands over the next batch's pieces a few microseconds after the last ones were done: look for them
      // for a moment before going to sleep (waking a sleeping thread costs more than a piece takes to copy).
      for (int spin = 0; spin < 4000 && !have; spin++) {
        if (pending_.load(std::memory_order_acquire)) {
          std::lock_guard<std::mutex> g(mu_);
          if (!queue_.empty()) { t = queue_.back(); queue_.pop_back(); pending_.fetch_sub(1, std::memory_order_relaxed); have = true; }
        } else {
          _mm_pause();
        }
      }
      if (!have) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !queue_.empty(); });
        if (stop_ && queue_.empty()) return;
        t = queue_.back(); queue_.pop_back(); pending_.fetch_sub(1, std::memory_order_relaxed);
      }
      do_task(t);
    }
  }
  std::atomic<int> pending_{0};
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Task> queue_;
  bool stop_ = false;
};

// Layout of one batch's packed input image: the same bytes in the slot's pinned buffer and in HBM.  Offsets are into
// the image; blobs start 64-byte aligned and are followed by 64 bytes of slack (the kernels read 16 bytes at a time).
struct ImageLayout {
  size_t raw_off, dom_off, key_off, key_type, ext_null, cap_off, cap_str_off, raw, dom, key, cap_blob, total;
  size_t mixed;       // a mixed regex batch's plan (mixed_plan.hip.h, MixedImage) and, behind it, a mixed extraction's tables (CapMixedImage); no bytes otherwise
};
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }
inline ImageLayout image_layout(uint32_t n, size_t raw_total, size_t dom_total, size_t key_total, size_t n_cap_off, size_t n_cap_str,
                                size_t cap_bytes, size_t mixed_bytes = 0) {
  ImageLayout L{};
  size_t o = 0;
  auto put = [&](size_t bytes, size_t slack) { const size_t at = o; o = align_up(o + bytes + slack, 64); return at; };
  L.raw_off = put((size_t)(n + 1) * 8, 0);
  L.dom_off = put((size_t)(n + 1) * 8, 0);
  L.key_off = put((size_t)(n + 1) * 8, 0);
  L.key_type = put(n, 0);
  L.ext_null = put(n, 0);
  L.cap_off = put(n_cap_off * 4, 0);
  L.cap_str_off = put(n_cap_str * 4, 0);
  L.mixed = put(mixed_bytes, 0);
  L.raw = put(raw_total, 64);
  L.dom = put(dom_total, 64);
  L.key = put(key_total, 64);
  L.cap_blob = put(cap_bytes, 64);
  L.total = o;
  return L;
}

// The buffers of one capture extraction (a slot's, or zke_capture_batch's own): spans, flags, codes and the three tables in one
// device buffer laid out by `L` (dfa_registry.hip.h, CapLayout) with a pinned twin of everything in front of the blob, and the rows
// of programs too large for LDS.
struct CapBufs {
  TwinBuf t;
  DevBuf work;
  CapLayout L{};
  void release() { t.release(); work.release(); }
};
template <class F> void each_buffer(CapBufs& b, F& f) { each_buffer(b.t, f); f(b.work); }

// The buffers of one signature scan (a slot's): {counter | statuses | record slots | selector blob} in one device buffer with a
// pinned twin of the same layout — the whole of it comes back as ONE copy —, and the overflow of the header span tables.
struct ScanLayout { size_t status, recs, blob, blob_cap, total; uint32_t n, max_sigs; };
inline ScanLayout scan_layout(uint32_t n, uint32_t max_sigs, size_t blob_cap) {
  ScanLayout L{};
  L.n = n; L.max_sigs = max_sigs; L.blob_cap = blob_cap;
  L.status = 64;                                                        // [0, 64): the selector bytes reserved so far
  L.recs = align_up(L.status + (size_t)n * 16, 64);
  L.blob = align_up(L.recs + (size_t)n * max_sigs * sizeof(zke_sig_info), 64);
  L.total = L.blob + blob_cap;
  return L;
}
struct ScanBufs {
  TwinBuf t;
  DevBuf ovf;
  ScanLayout L{};
};
template <class F> void each_buffer(ScanBufs& b, F& f) { each_buffer(b.t, f); f(b.ovf); }

// The buffers of one key-record decode (a slot's): {infos | decoded keys at their records' offsets} in one device buffer with a pinned
// twin — ONE copy back —, and, for zke_select_keys_from_records, the key section the front end reads: {key_off | key_type | packed blob}.
struct KeyrecLayout { size_t keys, total; uint32_t m; size_t p_type, p_blob, p_total; };
inline KeyrecLayout keyrec_layout(uint32_t m, size_t rec_total) {
  KeyrecLayout L{};
  L.m = m;
  L.keys = align_up((size_t)m * sizeof(zke_key_info), 64);
  L.total = L.keys + rec_total;
  L.p_type = align_up(((size_t)m + 1) * 8, 64);
  L.p_blob = align_up(L.p_type + m, 64);
  L.p_total = L.p_blob + rec_total + 64;               // (a decoded key is shorter than its record; the kernels read 16 bytes at a time)
  return L;
}
struct KeyrecBufs {
  TwinBuf t;
  DevBuf pack;
  KeyrecLayout L{};
};
template <class F> void each_buffer(KeyrecBufs& b, F& f) { each_buffer(b.t, f); f(b.pack); }

// The buffers of one body extraction (a slot's; zke_extract_bodies): {infos | first places | second places} in one device buffer
// with a pinned twin.  E-mail i decodes into the first place at its raw offset; only a quoted-printable body that outgrows its e-mail
// (lone LF line ends become CRLF) goes on in the second place at the same offset (bodyext.hip.h).  ONE copy brings {infos | first
// places} back; the second places follow in a copy of their own when an info says one is in use (first_copy, then the rest).
struct BodyLayout { size_t bytes, region, first_copy, total; uint32_t n; };
inline BodyLayout body_layout(uint32_t n, size_t raw_total) {
  BodyLayout L{};
  L.n = n;
  L.bytes = align_up((size_t)n * sizeof(zke_body_info), 64);
  L.region = align_up(raw_total, 64);
  L.first_copy = L.bytes + L.region;
  L.total = L.first_copy + L.region;
  return L;
}
struct BodyBufs {
  TwinBuf t;
  DevBuf ovf;
  BodyLayout L{};
};
template <class F> void each_buffer(BodyBufs& b, F& f) { each_buffer(b.t, f); f(b.ovf); }
// The compaction of a finished extraction, host code only, in two steps around the one copy that may lie between them.
// body_measure: the device's infos (body_off = the e-mail's raw offset, reserved = its raw length: its place) checked against the
// layout — an info that points outside its place is refused, nothing is read through it — and delivered with body_off rewritten to
// the packed offsets; bytes_need; `spilled`: some body uses its second place.  0, ZKE_E_DEVICE (an info the kernel cannot have
// written) or ZKE_E_NOMEM (bytes is too small; the infos are delivered all the same).
inline int body_measure(const BodyLayout& K, const uint8_t* twin, zke_body_out* o, bool& spilled) {
  const zke_body_info* src = reinterpret_cast<const zke_body_info*>(twin);
  spilled = false;
  for (uint32_t i = 0; i < K.n; i++) {
    const zke_body_info& f = src[i];
    const uint64_t len = f.status == ZKE_OK ? f.body_len : 0;
    if (f.body_off > K.region || f.reserved > K.region - f.body_off || len > 2 * (uint64_t)f.reserved) return ZKE_E_DEVICE;
  }
  size_t total = 0;
  for (uint32_t i = 0; i < K.n; i++) {
    zke_body_info f = src[i];
    if (f.status != ZKE_OK) f.body_len = 0;
    spilled = spilled || f.body_len > f.reserved;
    f.body_off = total; f.reserved = 0;
    total += f.body_len;
    o->infos[i] = f;
  }
  o->bytes_need = total;
  return total > o->bytes_cap ? ZKE_E_NOMEM : 0;
}
// body_compact: behind a body_measure that returned 0 (and, when it said `spilled`, the copy of the second places): one memcpy per
// body, two for a spilled one.
inline void body_compact(const BodyLayout& K, const uint8_t* twin, zke_body_out* o) {
  const zke_body_info* src = reinterpret_cast<const zke_body_info*>(twin);
  for (uint32_t i = 0; i < K.n; i++) {
    const size_t len = o->infos[i].body_len, cap = src[i].reserved, at = (size_t)src[i].body_off;
    if (!len) continue;
    uint8_t* dst = o->bytes + o->infos[i].body_off;
    const size_t a = std::min(len, cap);
    memcpy(dst, twin + K.bytes + at, a);
    if (len > a) memcpy(dst + a, twin + K.first_copy + at, len - a);
  }
}

// The origins of one mapped extraction (a slot's; zke_extract_captures_mapped): {spans n*G*2 | flags n*G} in a device buffer of its own
// with a pinned twin — a plain extraction never sees it.  `launched`: capture_origin_kernel ran for the pending batch (it does not
// when no body part asks for a group: the origins are then the spans themselves).
struct OriginLayout { size_t flags, total; size_t NG; };
inline OriginLayout origin_layout_sized(size_t NG) {      // NG columns: n * G, or a mixed extraction's Gt
  OriginLayout L{};
  L.NG = NG;
  L.flags = align_up(L.NG * 8, 64);
  L.total = align_up(L.flags + L.NG, 64);
  return L;
}
inline OriginLayout origin_layout(uint32_t n, uint32_t G) { return origin_layout_sized((size_t)n * G); }
struct OriginBufs {
  TwinBuf t;
  OriginLayout L{};
  bool launched = false;
};
template <class F> void each_buffer(OriginBufs& b, F& f) { each_buffer(b.t, f); }

// The buffers of one output encoding (a slot's; zke_verify_emails_encoded, zke_encode_outputs; kernel: encode.hip.h): {infos |
// encodings} in one device buffer with a pinned twin — that prefix comes back as ONE copy — and behind it, on the device alone, the
// digest launch's job list.  `blob`: the planned bytes of the encodings (encode_plan.hip.h), exact.  `in`: the building block's
// staged records and tables (the verify entry's ride in the batch's input image: EncImage).
struct EncLayout { size_t bytes, prefix, sha, total; uint64_t blob; uint32_t n; };
inline EncLayout enc_layout(uint32_t n, uint64_t blob) {
  EncLayout L{};
  L.n = n; L.blob = blob;
  L.bytes = align_up((size_t)n * sizeof(zke_encoded_info), 64);
  L.prefix = L.bytes + (size_t)blob;
  L.sha = align_up(L.prefix, 64);
  L.total = L.sha + (size_t)n * sizeof(ShaJob);
  return L;
}
// A device-planned encoding (zke_extract_captures_encoded): `blob` is the CAPACITY of the encodings — their size is known only
// once the batch has run —, the plan's jobs lie behind the digest jobs, and the pinned twin holds the infos alone: the bytes come
// back in a copy of their own, of exactly the size the infos name (deliver_encoded_planned).
inline EncLayout enc_layout_planned(uint32_t n, uint64_t blob_cap, size_t& jobs_at) {
  EncLayout L = enc_layout(n, blob_cap);
  jobs_at = align_up(L.total, 64);
  L.total = jobs_at + (size_t)n * sizeof(EncodeJob);
  return L;
}
struct EncBufs {
  TwinBuf t;
  DevBuf in;
  EncLayout L{};
  size_t jobs_at = 0;        // (a device-planned encoding)
};
template <class F> void each_buffer(EncBufs& b, F& f) { each_buffer(b.t, f); f(b.in); }
// What the encode launch reads besides the records and the capture tables, as one section of a batch's input image: the jobs and the
// external-input table (offsets into the section; the blob 64-byte aligned like the image's others).
struct EncImage { size_t jobs, ext_str_off, ext_blob, total; };
inline EncImage enc_image(uint32_t n, uint32_t ext_strs, uint32_t ext_bytes) {
  EncImage L{};
  L.jobs = 0;
  L.ext_str_off = align_up((size_t)n * sizeof(EncodeJob), 64);
  L.ext_blob = align_up(L.ext_str_off + (ext_strs ? (size_t)ext_strs + 1 : 0) * 4, 64);
  L.total = align_up(L.ext_blob + ext_bytes, 64);
  return L;
}

// ---- The plan sections of a batch's image: tables built on the host that ride behind ImageLayout::mixed, one behind the other — a
// mixed batch's plan, a mixed extraction's tables, an encoding's jobs and external inputs (which start 64-byte aligned: a blob lies
// in them).  A section is a layout (mixed_image, capmix_image, enc_image), a stage_* that copies the plan's arrays to their places
// from the section's base in the pinned image, and a *_view that names the same places from its base in HBM: a section's offsets are
// used by those two and nobody else.  Plain C++ like the layouts: no HIP call, no engine.  A section that is not there has no bytes.
struct PlanSections {
  MixedImage mixed{}; CapMixedImage capmix{}; EncImage enc{};
  size_t capmix_at = 0, enc_at = 0, total = 0;      // mixed lies at 0; offsets from ImageLayout::mixed
};
inline PlanSections plan_sections(const MixedImage& mixed, const CapMixedImage& capmix, const EncImage& enc) {
  PlanSections S{mixed, capmix, enc};
  S.capmix_at = mixed.total;
  S.enc_at = align_up(S.capmix_at + capmix.total, 64);
  S.total = S.enc_at + enc.total;
  return S;
}

// The plan of a mixed batch and where its tables lie in the slot's staged image (device pointers).
struct MixedLaunch {
  const MixedPlan* plan;
  const uint32_t* job_off; const uint32_t* email_cfg; const uint32_t* perm; const MixedSeg* segs;
};
inline void stage_mixed(uint8_t* base, const MixedImage& L, const MixedPlan& P) {
  stage_copy(base + L.job_off, P.job_off.data(), P.job_off.size() * 4);
  stage_copy(base + L.email_cfg, P.email_cfg.data(), P.email_cfg.size() * 4);
  stage_copy(base + L.perm, P.perm.data(), P.perm.size() * 4);
  stage_copy(base + L.segs, P.segs.data(), P.segs.size() * sizeof(MixedSeg));
}
inline MixedLaunch mixed_view(const uint8_t* base, const MixedImage& L, const MixedPlan* plan) {
  return MixedLaunch{plan, reinterpret_cast<const uint32_t*>(base + L.job_off), reinterpret_cast<const uint32_t*>(base + L.email_cfg),
                     reinterpret_cast<const uint32_t*>(base + L.perm), reinterpret_cast<const MixedSeg*>(base + L.segs)};
}

// The shape of a mixed extraction and where its tables lie in the slot's staged image (device pointers).
struct CapMixedLaunch {
  uint32_t J, Gt;
  bool needs_work;              // some part of some config keeps its rows in the slot's workspace: the grid is bounded by CAP_WORK_WAVES
  bool origin;                  // the origin launch runs (org is wanted and some body part asks for a group)
  CapMixedTables t;
};
// `part`: the config-major part table as the registry resolved it (the plan's shape.n_parts entries)
inline void stage_capmix(uint8_t* base, const CapMixedImage& L, const CapMixedPlan& P, const std::vector<CapPartDev>& part) {
  stage_copy(base + L.col_off, P.col_off.data(), P.col_off.size() * 4);
  stage_copy(base + L.cap_cfg, P.cap_cfg.data(), P.cap_cfg.size() * 4);
  stage_copy(base + L.cfgs, P.cfgs.data(), P.cfgs.size() * sizeof(CapMixedCfg));
  stage_copy(base + L.parts, part.data(), part.size() * sizeof(CapPartDev));
}
// job_off: the mixed plan's, in its own section (mixed_view)
inline CapMixedTables capmix_view(const uint8_t* base, const CapMixedImage& L, const uint32_t* job_off) {
  return CapMixedTables{job_off, reinterpret_cast<const uint32_t*>(base + L.col_off), reinterpret_cast<const uint32_t*>(base + L.cap_cfg),
                        reinterpret_cast<const CapMixedCfg*>(base + L.cfgs), reinterpret_cast<const CapPartDev*>(base + L.parts)};
}

// An encoding's section.  A host plan stages its jobs; a device plan (zke_extract_captures_encoded) has none yet, and ext_off[n + 1]
// rides in their place when there are external inputs at all.  The external-input table is the caller's either way.
inline void stage_enc(uint8_t* base, const EncImage& L, const EncodePlan& P, bool device_plan, const uint32_t* ext_off, uint32_t n,
                      const uint32_t* ext_str_off, const uint8_t* ext_blob) {
  if (!device_plan) stage_copy(base + L.jobs, P.jobs.data(), P.jobs.size() * sizeof(EncodeJob));
  else if (P.ext_strs) stage_copy(base + L.jobs, ext_off, ((size_t)n + 1) * 4);
  if (P.ext_strs) stage_copy(base + L.ext_str_off, ext_str_off, ((size_t)P.ext_strs + 1) * 4);
  if (P.ext_bytes) stage_copy(base + L.ext_blob, ext_blob, P.ext_bytes);
}
// The input half of the encode launch's arguments that the section holds (a device plan: `jobs` points to ext_off, see above).
inline EncodeArgs enc_view(const uint8_t* base, const EncImage& L) {
  EncodeArgs a{};
  a.jobs = reinterpret_cast<const EncodeJob*>(base + L.jobs);
  a.ext_str_off = reinterpret_cast<const uint32_t*>(base + L.ext_str_off); a.ext_blob = base + L.ext_blob;
  return a;
}

// The buffers of zke_qp_clean_batch (a slot's): the bodies and their offsets, cleaned bytes, index map, kept lengths.
struct QpBufs { DevBuf in, off, clean, map, len; };
template <class F> void each_buffer(QpBufs& b, F& f) { for (DevBuf* x : {&b.in, &b.off, &b.clean, &b.map, &b.len}) f(*x); }

// The buffers of zke_utf8_lossy_batch (a slot's): the strings and their offsets, the repaired offsets, bytes and flags.
struct Utf8Bufs { DevBuf in, off, out_off, out, flags; };
template <class F> void each_buffer(Utf8Bufs& b, F& f) { for (DevBuf* x : {&b.in, &b.off, &b.out_off, &b.out, &b.flags}) f(*x); }

// What a slot owes the caller of its pending host batch: where each output goes once the batch's last copy has arrived.  A
// default-constructed one owes nothing.  submit_host files it (pending_delivery), retire_host takes it out whole, deliver_pending
// pays it (host_entry.hip.h).
struct PendingDelivery {
  zke_result* records = nullptr;       // the records as they are (a verify batch, an extraction) ...
  uint32_t n = 0;
  std::vector<uint32_t> sel_off;       // ... or folded per e-mail: cand_off of a key selection, rebased to 0 (n + 1 entries; empty: no selection)
  zke_result* sel_out = nullptr;
  uint32_t* sel_chosen = nullptr;
  zke_sig_scan* scan = nullptr;
  zke_keyrec_out* keyrec = nullptr;
  zke_body_out* body = nullptr;
  zke_capture_out* caps = nullptr;
  zke_capture_origin* org = nullptr;   // (with caps only: a mapped extraction)
  zke_encoded_out* enc = nullptr;      // (beside the records: zke_verify_emails_encoded)
  bool enc_planned = false;            // (with enc: the plan was the device's — zke_extract_captures_encoded; caps may then be null)
};

}  // namespace
