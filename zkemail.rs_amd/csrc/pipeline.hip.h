// pipeline.hip.h — host orchestration of one batch: workspace sizing, the kernel sequence of
// verify_email / verify_email_with_regex (core/src/circuits.rs:9-68), the submission entry points (device-resident and
// host-memory batches), DFA registration.  Included by engine.hip (single translation unit).
#pragma once

namespace {

inline uint64_t host_scratch_off(const uint64_t* raw_off, uint32_t i) { return scratch_offset(raw_off[i] - raw_off[0], i); }

struct StageTimer {
  Slot* w; hipStream_t s; bool on;
  StageTimer(zke_engine* e_, Slot* w_, hipStream_t s_) : w(w_), s(s_), on(e_->timing.load()) {}
  void mark(int k) { if (on && hipEventRecord(w->ev[k], s) == hipSuccess) w->marks |= 1u << k; }
};

// Length-bucket counters start a batch at zero (the verdict launch of the slot's previous batch clears them): a fresh
// allocation is cleared here.
int ensure_zeroed(DevBuf& b, size_t need) {
  const void* old = b.p;
  if (int r = b.ensure(need)) return r;
  if (b.p != old && hipMemset(b.p, 0, b.cap) != hipSuccess) return ZKE_E_DEVICE;
  return 0;
}

// Workspace of one slot for batches of up to n e-mails / raw_total raw bytes (P regex parts; with_regex: the buffers of
// the canonicalize_signed_email pass too).  Grows only: in steady state — or after zke_engine_reserve — this allocates nothing.
int ensure_workspace(zke_engine* e, Slot& w, uint32_t n, uint64_t raw_total, bool with_regex, uint32_t P, bool want_em) {
  const uint32_t n_pad = (n + 63) & ~63u;
  int r = 0;
  const size_t scratch_bytes = 2 * (size_t)raw_total + (size_t)(n + 1) * SCR_PER_EMAIL + 256;
  if ((r = w.meta.ensure((size_t)n * sizeof(EmailMeta))) || (r = w.rsa_jobs.ensure((size_t)n * sizeof(RsaJob))) ||
      (r = w.sha_jobs.ensure((size_t)4 * n_pad * sizeof(ShaJob))) || (r = w.rsa_ok.ensure((size_t)n * 4)) ||
      (r = ensure_zeroed(w.sha_order, (size_t)2 * (SHA_ORDER_KIND_WORDS + n_pad) * 4)) ||
      (r = w.scratch_off.ensure((size_t)(n + 1) * 16)) || (r = w.scratch.ensure(scratch_bytes)))
    return fail(e, r, "workspace allocation");
  if (!w.pending.p) {       // counters: [0] e-mails pending another signature round, [2] length of the wave-routine job list (rsa_ok)
    if ((r = w.pending.ensure(64))) return fail(e, r, "workspace allocation");
    HIPCHK(e, hipMemset(w.pending.p, 0, 64));
  }
  if (want_em && (r = w.em_dbg.ensure((size_t)n * 512))) return fail(e, r, "workspace allocation");
  if (with_regex) {
    if ((r = w.meta2.ensure((size_t)n * sizeof(EmailMeta))) || (r = w.scratch2.ensure(scratch_bytes)) ||
        (r = w.clean.ensure((size_t)raw_total + (size_t)(n + 1) * CLEAN_PER_EMAIL + 256)) ||
        (r = w.parts.ensure((size_t)n * std::max<uint32_t>(P, 1) * sizeof(PartRes))))
      return fail(e, r, "workspace allocation");
  }
  return 0;
}

// Host-entry buffers of one slot: the packed input image (pinned and in HBM) and the records (HBM and pinned).
int ensure_host_buffers(zke_engine* e, Slot& w, size_t image_bytes, uint32_t n) {
  int r = 0;
  if ((r = w.h_image.ensure(image_bytes)) || (r = w.d_image.ensure(image_bytes)) ||
      (r = w.h_results.ensure((size_t)n * sizeof(zke_result))) || (r = w.d_results.ensure((size_t)n * sizeof(zke_result))))
    return fail(e, r, "host-entry staging allocation");
  return 0;
}

// (caller holds reg_mu exclusively or is creating the engine)
int raise_dfa_lds_attrs(zke_engine* e, size_t lds) {
  if (lds > e->dfa_wave_lds_attr) {
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&dfa_wave_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    e->dfa_wave_lds_attr = lds;
  }
  if (lds > e->dfa_lds_attr) {
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&dfa_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    e->dfa_lds_attr = lds;
  }
  return 0;
}

int arg_error(const char* who, const char* what);

// ---- capture extraction behind the regex stage (capture.hip.h)
// An extraction riding on a regex batch: the parts' programs and requested groups, resolved against the registry.
struct CaptureReq {
  uint32_t P = 0, G = 0, n_header_parts = 0;
  bool needs_work = false;               // some program's rows do not fit LDS
  CapPartDev part[CAP_MAX_PARTS]{};
  uint32_t gbase[CAP_MAX_PARTS + 1]{};
  std::vector<uint32_t> dfa_ids;         // [P] header parts, then body parts
  uint32_t prog_ids[CAP_MAX_PARTS]{};    // resolved against the registry by capture_resolve, under the engine's `big` lock
  zke_capture_out* out = nullptr;
};
constexpr uint32_t CAP_WORK_WAVES = 256;      // waves of a capture launch whose rows live in the slot's workspace (one slice each)

int ensure_capture_buffers(zke_engine* e, CapBufs& b, uint32_t n, uint32_t P, uint32_t G, size_t blob_cap, bool work) {
  const CapLayout L = cap_layout(n, P, G, blob_cap);
  int r = 0;
  if ((r = b.cap.ensure(L.total)) || (r = b.h_cap.ensure(L.fixed_end)) ||
      (work && (r = b.work.ensure((size_t)CAP_WORK_WAVES * CAP_WORK_WORDS * 8))))
    return fail(e, r, "capture workspace allocation");
  return 0;
}

// Part p of a request: the requested groups (no registry involved: the sizes of the output follow from these alone) ...
int capture_part_shape(CaptureReq& q, uint32_t p, uint32_t prog_id, const uint32_t* groups, uint32_t n_groups, const char* who) {
  if (n_groups > ZKE_CAP_MAX_GROUPS) return arg_error(who, "more than ZKE_CAP_MAX_GROUPS groups requested for a part");
  if (n_groups && !groups) return arg_error(who, "null group list");
  CapPartDev& d = q.part[p];
  d = CapPartDev{};
  d.code = ZKE_D_U_CAPTURE_PROGRAM;
  d.n_groups = n_groups; d.gbase = q.gbase[p];
  for (uint32_t k = 0; k < n_groups; k++) d.groups[k] = groups[k];
  q.prog_ids[p] = prog_id;
  q.gbase[p + 1] = q.gbase[p] + n_groups;
  q.G = q.gbase[p + 1];
  return 0;
}
// ... and the programs' device tables.  The caller holds `big` (shared) from here until the batch is enqueued: unregistering a
// program takes `big` exclusively and drains the engine before it frees a table, so the pointers copied here stay valid for as
// long as a launch can read them — the same order in which run_device_pipeline resolves the DFA pairs of a batch.
void capture_resolve(zke_engine* e, CaptureReq& q) {
  std::shared_lock<std::shared_mutex> rl(e->reg_mu);
  q.needs_work = false;
  for (uint32_t p = 0; p < q.P; p++) {
    CapPartDev& d = q.part[p];
    const uint32_t id = q.prog_ids[p];
    const RegisteredCapture* rc = id < e->captures.size() ? e->captures[id] : nullptr;
    d.code = rc ? rc->detail : (uint32_t)ZKE_D_U_CAPTURE_PROGRAM;
    d.prog = CapProgDev{};
    if (rc && !rc->detail) { d.prog = rc->dev; if (d.prog.words64 > CAP_LDS_WORDS) q.needs_work = true; }
  }
}

// The two launches of an extraction: the walk per (e-mail, part), then verdict + tables.  `parts`: the PartRes the search left.
int launch_capture(zke_engine* e, CapBufs& b, const CaptureReq& q, uint32_t n, bool plain, const DfaArgs& base,
                   const uint8_t* hay_blob, const uint64_t* hay_off, const PartRes* parts, zke_result* results, hipStream_t s) {
  const CapLayout& L = b.L;
  uint8_t* cb = b.cap.as<uint8_t>();
  CapArgs ca{};
  ca.plain = plain ? 1u : 0u; ca.n = n; ca.P = q.P; ca.G = q.G; ca.d = base; ca.n_header_parts = q.n_header_parts;
  ca.hay_blob = hay_blob; ca.hay_off = hay_off; ca.parts = parts;
  ca.spans = reinterpret_cast<uint32_t*>(cb + L.spans); ca.flags = cb + L.flags; ca.codes = reinterpret_cast<uint32_t*>(cb + L.codes);
  ca.work = b.work.as<uint64_t>();
  for (uint32_t p = 0; p < q.P; p++) ca.part[p] = q.part[p];
  const uint32_t items = n * q.P;
  const uint32_t grid = std::min<uint32_t>(items, q.needs_work ? CAP_WORK_WAVES : 16384u);
  if (grid) hipLaunchKernelGGL(capture_kernel, dim3(grid), dim3(64), 0, s, ca);
  CapGatherArgs ga{};
  ga.plain = ca.plain; ga.n = n; ga.P = q.P; ga.G = q.G; ga.n_header_parts = q.n_header_parts; ga.d = base;
  ga.hay_blob = hay_blob; ga.hay_off = hay_off; ga.parts = parts; ga.codes = ca.codes; ga.spans = ca.spans; ga.results = results;
  ga.cap_off = reinterpret_cast<uint32_t*>(cb + L.cap_off); ga.cap_str_off = reinterpret_cast<uint32_t*>(cb + L.cap_str_off);
  ga.cap_blob = cb + L.blob; ga.blob_cap = L.blob_cap; ga.hdr = reinterpret_cast<uint64_t*>(cb + L.hdr);
  ga.tmp = reinterpret_cast<uint32_t*>(cb + L.tmp);
  for (uint32_t p = 0; p <= q.P; p++) ga.gbase[p] = q.gbase[p];
  hipLaunchKernelGGL(capture_gather_kernel, dim3(1), dim3(1024), 0, s, ga);
  HIPCHK(e, hipGetLastError());
  return 0;
}

// The device pipeline.  Every pointer in `in` / out_dev is device memory, except the part-id lists (host arrays in both
// entry points).  Three launches — front end, hash / modexp stage, Ed25519 + verdict (which also runs the later signature
// rounds of the rare e-mail that needs them) — and, for verify_email_with_regex, the regex stage behind them.
// Caller holds the slot's lock; everything the call needs is in its arguments or in the slot.
// ---- signature scan and key selection (sigscan.hip.h; include/zkemail_amd.h)
struct ScanReq { uint32_t max_sigs; zke_sig_scan* out; };
struct SelectReq { const uint32_t* cand_off; uint32_t n; zke_result* out; uint32_t* chosen; };
// ---- key records (keyrec.hip.h).  Alone: the batch's "raw e-mails" are the records, keyrec_kernel runs instead of the verify
// pipeline.  With a SelectReq: the image's key section holds the records, and the decode + pack launches in front of the front end
// replace it by the decoded keys (zke_select_keys_from_records).
struct KeyrecReq { uint32_t mode; zke_keyrec_out* out; };

int ensure_keyrec_buffers(zke_engine* e, KeyrecBufs& b, uint32_t m, size_t rec_total, bool pack) {
  const KeyrecLayout L = keyrec_layout(m, rec_total);
  int r = 0;
  if ((r = b.out.ensure(L.total)) || (r = b.h_out.ensure(L.total)) || (pack && (r = b.pack.ensure(L.p_total))))
    return fail(e, r, "key-record buffer allocation");
  b.L = L;
  return 0;
}

// A slot's scan buffers for n e-mails with max_sigs record slots each and blob_cap bytes of selectors.  Grow only: the first scan
// of a shape allocates, a later one of the same shape does not.
int ensure_scan_buffers(zke_engine* e, ScanBufs& b, uint32_t n, uint32_t max_sigs, size_t blob_cap) {
  const ScanLayout L = scan_layout(n, max_sigs, blob_cap);
  int r = 0;
  if ((r = b.out.ensure(L.total)) || (r = b.h_out.ensure(L.total)) || (r = b.ovf.ensure((size_t)n * HDR_OVF_BYTES)))
    return fail(e, r, "signature-scan buffer allocation");
  b.L = L;
  return 0;
}

int run_device_pipeline(zke_engine* e, Slot& w, const zke_batch* in, uint64_t raw_total, uint64_t key_total, zke_result* out_dev,
                        hipStream_t s, bool want_em, uint64_t now, bool want_clean = false, const CaptureReq* cap = nullptr) {
  const uint32_t n = in->n;
  if (n == 0) return 0;
  const uint32_t n_pad = (n + 63) & ~63u;
  const uint32_t P = in->with_regex ? in->n_header_parts + in->n_body_parts : 0;
  int r = 0;
  if ((r = ensure_workspace(e, w, n, raw_total, in->with_regex != 0, P, want_em))) return r;
  uint64_t* scratch_off = w.scratch_off.as<uint64_t>();
  uint64_t* clean_off = scratch_off + (n + 1);

  StageTimer tm(e, &w, s);
  if (!(w.marks & (1u << MK_START))) tm.mark(MK_START);      // (the host entry has marked the start in front of its H2D)
  // (offsets, padding SHA jobs and the pending counter are initialised by the round-0 front-end kernel: batch_prologue)

  BatchDev B{};
  B.n = n;
  B.raw = in->raw_blob; B.raw_off = in->raw_off;
  B.dom = in->domain_blob; B.dom_off = in->domain_off;
  B.key = in->key_blob; B.key_off = in->key_off;
  B.key_type = in->key_type; B.ext_null = in->ext_null;
  B.results = out_dev;
  B.meta = w.meta.as<EmailMeta>();
  B.rsa = w.rsa_jobs.as<RsaJob>();
  B.sha = w.sha_jobs.as<ShaJob>();
  B.n_pad = n_pad;
  B.scratch = w.scratch.as<uint8_t>();
  B.scratch_off = scratch_off;
  B.clean_off = clean_off;
  B.pending = w.pending.as<uint32_t>();
  B.meta_verify = nullptr;
  B.order = n < (1u << 24) ? w.sha_order.as<uint32_t>() : nullptr;      // a key holds the position within a class in 24 bits

  const uint32_t rounds = e->opt.max_sig_rounds;
  // an RSA-2048 key is 270 bytes of DER: a batch whose keys average more holds some larger modulus
  const uint32_t route_mask = rsa_route_mask(e, n, key_total > (uint64_t)n * 272);
  {
    const uint32_t round = 0;
    uint32_t* wave_count = w.pending.as<uint32_t>() + 2;
    uint32_t* wave_list = w.rsa_ok.as<uint32_t>();
    ParseArgs pa{B, round, 0, e->debug_parse_stop, e->strict, now, e->key_cache.as<KeyCacheEntry>(), route_mask, wave_count, wave_list};
    hipLaunchKernelGGL(parse_kernel, dim3((n + ZKE_PARSE_WG_WAVES - 1) / ZKE_PARSE_WG_WAVES), dim3(64 * ZKE_PARSE_WG_WAVES), PARSE_DYN_LDS, s, pa);
    tm.mark(MK_FRONT);
    // hash / modexp stage: the four SHA-256 jobs and the RSA operation of every e-mail, one launch (fused.hip.h)
    if (!(e->debug_skip_launch & 1) &&
        (r = launch_hash_modexp(e, B.sha, 4 * n_pad, B.rsa, n, B.meta, want_em ? w.em_dbg.as<uint8_t>() : nullptr, route_mask, wave_count, wave_list, B.order,
                                __atomic_load_n(w.wave_feedback, __ATOMIC_RELAXED), s)))
      return r;
    tm.mark(MK_HASH);
    // Ed25519 stage + verdicts (verdict.hip.h): bh compare, EM digest against the header hash, status / detail, pending counter
    EdVerdictArgs va{FinArgs{B, round, rounds, w.pending.as<uint32_t>(), e->debug_skip_rsa}, e->debug_skip_ed, wave_count,
                     e->key_cache.as<KeyCacheEntry>(), want_em ? w.em_dbg.as<uint8_t>() : nullptr, e->strict, now, w.wave_feedback};
    if (!(e->debug_skip_launch & 2)) hipLaunchKernelGGL(ed_verdict_kernel, dim3((n + VERDICT_EMAILS_PER_WAVE - 1) / VERDICT_EMAILS_PER_WAVE), dim3(64), 0, s, va);
    tm.mark(MK_VERDICT);
  }
  HIPCHK(e, hipGetLastError());

  if (in->with_regex) {
    // the parts of this batch, copied out of the registry (the entries themselves stay put until the engine is idle)
    PartInfo parts_small[16];
    std::vector<PartInfo> parts_big;
    PartInfo* parts = parts_small;
    if (P > 16) { parts_big.resize(P); parts = parts_big.data(); }
    {
      std::shared_lock<std::shared_mutex> rl(e->reg_mu);
      for (uint32_t p = 0; p < P; p++) {
        const uint32_t id = p >= in->n_header_parts ? in->body_part_ids[p - in->n_header_parts] : in->header_part_ids[p];
        PartInfo pi{};
        const RegisteredDfa* rd = id < e->dfas.size() ? e->dfas[id] : nullptr;
        if (rd) {
          pi.detail = rd->detail; pi.lds_bytes = rd->lds_bytes; pi.idle = rd->idle;
          pi.dev = rd->valid ? rd->dev.as<RegexDev>() : nullptr;
        }
        parts[p] = pi;
      }
    }
    // canonicalize_signed_email (circuits.rs:34-35: first DKIM-Signature header, own scratch unless it is the verified one) and
    // remove_quoted_printable_soft_breaks (circuits.rs:37), one launch (regex.hip.h, regex_prep_kernel).  The cleaned body is
    // unobservable without body parts (circuits.rs:48-56): it is then only produced when a parity buffer asks for it.
    BatchDev B2 = B;
    B2.meta = w.meta2.as<EmailMeta>();
    B2.scratch = w.scratch2.as<uint8_t>();
    B2.meta_verify = B.meta;
    B2.order = nullptr;
    PrepArgs pr{ParseArgs{B2, 0, 1, 0, e->strict, now, nullptr, 0, nullptr, nullptr},
                QpArgs{B2, B.meta, w.clean.as<uint8_t>(), clean_off, B.scratch, B.scratch_off},
                (in->n_body_parts || want_clean) ? 1u : 0u};
    hipLaunchKernelGGL(regex_prep_kernel, dim3(n), dim3(64), 0, s, pr);
    tm.mark(MK_PREP);
    DfaArgs base{};
    base.b = B2; base.P = P;
    base.scratch_v = B.scratch; base.scratch_v_off = B.scratch_off;
    base.clean = w.clean.as<uint8_t>(); base.clean_off = clean_off;
    base.cap_off = in->cap_off; base.cap_str_off = in->cap_str_off; base.cap_blob = in->cap_blob;
    base.out = w.parts.as<PartRes>();
    auto part_lds = [&](const PartInfo& pi, uint32_t& in_lds) -> size_t {
      in_lds = 0;
      if (pi.dev && pi.lds_bytes + 1024 <= 150 * 1024) { in_lds = 1; return pi.lds_bytes + 1024; }
      return 1024;
    };
    // Which kernel: the wave-per-e-mail kernel shortens the chain (latency) but runs its serial part on one
    // lane's worth of work per wave, so it issues several times the instructions of the lane-per-e-mail kernel.
    // Body parts (KBs per e-mail) always gain; header parts (~1 KB) gain only while the batch is small enough for
    // latency to be what matters (measured: configs[2] shape, 4 096 per batch, 16.0 M e-mails/s with the lane kernel
    // against 12.7 M with the wave kernel; 1 024 per batch 11.4 M against 11.8 M).  zke_options.dfa_mapping forces one.
    const uint32_t wave_from = e->opt.dfa_mapping == 1 ? P : e->opt.dfa_mapping == 2 ? 0u
                             : (n <= 1024 ? 0u : in->n_header_parts);      // parts [wave_from, P) use the wave kernel
    // Parts in order, up to DFA_MULTI_MAX per launch (grid.y): [0, wave_from) one e-mail per lane, [wave_from, P) one e-mail per
    // wave.  A last launch that holds ONE part also writes the regex verdict into the records (it folds the earlier launches'
    // parts first); otherwise the verdict is a small launch of its own behind them.  (The parts of a launch run side by side:
    // walking them one after the other inside a block, verdict folded in, was measured — configs[4] shape 10.2 M e-mails/s
    // against 11.9 M, its dfa stage 505 us alone against 387.)
    bool folded = false;
    for (uint32_t p0 = 0; p0 < P;) {
      const bool lane_kernel = p0 < wave_from;
      const uint32_t end = lane_kernel ? wave_from : P;
      const uint32_t np = std::min<uint32_t>(DFA_MULTI_MAX, end - p0);
      DfaMultiArgs ma{};
      ma.common = base; ma.part0 = p0; ma.np = np; ma.n_header_parts = in->n_header_parts;
      ma.finalize = (p0 + np >= P && np == 1) ? 1u : 0u;
      folded = ma.finalize != 0;
      size_t lds = 1024;
      for (uint32_t k = 0; k < np; k++) {
        const PartInfo& pi = parts[p0 + k];
        ma.re[k] = pi.dev;
        lds = std::max(lds, part_lds(pi, ma.lds_tables[k]));
        ma.idle[k] = (pi.dev && !lane_kernel) ? pi.idle : 0xFFFFFFFFu;
        ma.detail[k] = pi.detail;
      }
      if (lane_kernel) hipLaunchKernelGGL(dfa_kernel, dim3((n + 255) / 256, np), dim3(256), lds, s, ma);
      else hipLaunchKernelGGL(dfa_wave_kernel, dim3((n + 3) / 4, np), dim3(256), lds, s, ma);
      p0 += np;
    }
    if (!folded) {
      RegexFinArgs rf{B2, w.parts.as<PartRes>(), in->n_header_parts, in->n_body_parts};
      hipLaunchKernelGGL(regex_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, s, rf);
    }
    // capture extraction (zke_extract_captures): two more launches behind the regex verdict, in the slot's capture buffer
    if (cap)
      if ((r = launch_capture(e, w.cb, *cap, n, false, base, nullptr, nullptr, w.parts.as<PartRes>(), out_dev, s))) return r;
    tm.mark(MK_DFA);
    HIPCHK(e, hipGetLastError());
  }
  return 0;
}

// Read the slot's timing marks (their events have completed) into w.last.
void collect_timings(Slot& w) {
  auto has = [&](int k) { return (w.marks >> k) & 1u; };
  auto dt = [&](int a, int b) { float ms = 0; if (hipEventElapsedTime(&ms, w.ev[a], w.ev[b]) != hipSuccess) return 0.f; return ms * 1000.f; };
  zke_timings t{};
  if (has(MK_START) && has(MK_FRONT) && has(MK_HASH) && has(MK_VERDICT)) {
    const int k0 = has(MK_H2D) ? MK_H2D : MK_START;          // where the first launch starts
    if (has(MK_H2D)) t.h2d_us = dt(MK_START, MK_H2D);
    t.front_end_us = dt(k0, MK_FRONT);
    t.hash_modexp_us = dt(MK_FRONT, MK_HASH);
    t.ed_verdict_us = dt(MK_HASH, MK_VERDICT);
    int klast = MK_VERDICT;
    if (has(MK_PREP) && has(MK_DFA)) { t.regex_prep_us = dt(MK_VERDICT, MK_PREP); t.dfa_us = dt(MK_PREP, MK_DFA); klast = MK_DFA; }
    t.total_us = dt(k0, klast);
    if (has(MK_D2H)) t.d2h_us = dt(klast, MK_D2H);
  }
  w.last = t;
  w.marks = 0;
}

// see zke_engine_reserve: 256 bytes of private memory per lane (the front end's spills are 116), never written to `sink`
__global__ void slot_warm_kernel(uint32_t* sink) {
  volatile uint32_t buf[512];
  for (int i = 0; i < 512; i++) buf[i] = (uint32_t)i * 2654435761u + threadIdx.x;
  uint32_t acc = 0;
  for (int i = 0; i < 512; i++) acc += buf[(i * 7 + threadIdx.x) & 511];
  if (acc == 0x12345678u && sink) *sink = acc;
}

// The slot's workspace is about to be overwritten by a batch on stream s: whatever ran in it before must be over.
// Same stream: stream order is enough.  Another stream: wait for the event recorded behind the previous batch.
int acquire_slot(zke_engine* e, Slot& w, hipStream_t s) {
  if (w.last_stream && w.last_stream != s) {
    // a batch on the slot's own stream leaves no event behind (release_slot): record it now, behind that batch —
    // waiting for `done` as it stood would order this batch behind nothing
    if (w.last_stream == w.stream) HIPCHK(e, hipEventRecord(w.done, w.stream));
    HIPCHK(e, hipStreamWaitEvent(s, w.done, 0));
  }
  w.marks = 0;
  return 0;
}
int release_slot(zke_engine* e, Slot& w, hipStream_t s) {
  // the event is needed only where the next user of the slot may sit on another stream: a caller-provided stream
  if (s != w.stream) HIPCHK(e, hipEventRecord(w.done, s));
  w.last_stream = s;
  return 0;
}
// A batch's use of a slot, from acquire to release.  The release runs on EVERY way out — also when a launch failed after
// others were enqueued: the slot's next user (and zke_engine_join / zke_engine_sync) must be ordered behind whatever did
// reach the stream, or its workspace is overwritten under a half-launched batch.
struct SlotUse {
  zke_engine* e; Slot& w; hipStream_t s; bool armed = false;
  SlotUse(zke_engine* e_, Slot& w_, hipStream_t s_) : e(e_), w(w_), s(s_) {}
  int acquire() { const int r = acquire_slot(e, w, s); armed = (r == 0); return r; }
  int release() { armed = false; return release_slot(e, w, s); }
  ~SlotUse() { if (armed) { const std::string keep = g_err; (void)release_slot(e, w, s); g_err = keep; } }      // the first error is the one reported
};

// The slot's next submission ticket (round-robin over the slots that exist: zke_engine_reserve only appends).
Slot& next_slot(zke_engine* e, uint32_t& index) {
  index = e->ticket.fetch_add(1, std::memory_order_relaxed) % (uint32_t)e->slots.size();
  e->last_slot.store(index, std::memory_order_relaxed);
  return *e->slots[index];
}
// tickets: slot index in the low 6 bits (an engine has at most 64 slots), the slot's batch count above
inline uint64_t make_ticket(uint32_t slot, uint64_t gen) { return (gen << 6) | slot; }

uint64_t batch_clock(const zke_engine* e) {
  if (!(e->strict & ZKE_STRICT_EXPIRY_X)) return 0;
  return e->opt.now_unix ? e->opt.now_unix : (uint64_t)time(nullptr);
}

// Deliver a host batch that was enqueued in this slot and not waited for yet: wait for its D2H, copy the records from the
// pinned buffer to the caller's `out`.  Caller holds the slot's lock.
// An extraction's tables from the slot's pinned twin (and the blob from HBM) into the caller's zke_capture_out.  Returns
// ZKE_E_NOMEM when the caller's cap_blob is too small for the strings (everything else is delivered; cap_blob_need says how much).
int deliver_captures(zke_engine* e, CapBufs& b, zke_capture_out* o, hipStream_t s) {
  const CapLayout& L = b.L;
  const uint8_t* hp = b.h_cap.as<uint8_t>();
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(hp + L.hdr);
  const size_t strings = (size_t)hdr[0], bytes = (size_t)hdr[1];
  memcpy(o->spans, hp + L.spans, o->spans_need * 4);
  memcpy(o->flags, hp + L.flags, o->flags_need);
  memcpy(o->cap_off, hp + L.cap_off, o->cap_off_need * 4);
  memcpy(o->cap_str_off, hp + L.cap_str_off, (strings + 1) * 4);
  o->n_strings = strings;
  o->cap_blob_need = bytes;
  const size_t take = std::min(bytes, L.blob_cap);
  if (take) {
    HIPCHK(e, hipMemcpyAsync(o->cap_blob, b.cap.as<uint8_t>() + L.blob, take, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  }
  if (bytes > L.blob_cap) return fail(e, ZKE_E_NOMEM, "capture extraction: cap_blob is smaller than the strings (zke_capture_out.cap_blob_need)");
  return 0;
}

// A scan from the slot's pinned twin into the caller's zke_sig_scan: statuses, the CSR over the record slots in use (the
// compaction: one memcpy per e-mail), the selector bytes.  ZKE_E_NOMEM when sigs or sel_blob is too small (*_need says how much).
int deliver_scan(zke_engine* e, const ScanBufs& b, zke_sig_scan* o) {
  const ScanLayout& S = b.L;
  const uint8_t* hp = b.h_out.as<uint8_t>();
  const uint32_t* st = reinterpret_cast<const uint32_t*>(hp + S.status);
  const zke_sig_info* recs = reinterpret_cast<const zke_sig_info*>(hp + S.recs);
  const size_t used = *reinterpret_cast<const uint32_t*>(hp);
  memcpy(o->scan_status, st, (size_t)S.n * 16);
  size_t total = 0;
  for (uint32_t i = 0; i < S.n; i++) { o->sig_off[i] = (uint32_t)total; total += std::min(st[4 * (size_t)i + 2], S.max_sigs); }
  o->sig_off[S.n] = (uint32_t)total;
  o->sigs_need = total; o->sel_blob_need = used; o->n_sigs = 0;
  if (total > o->sigs_cap) return fail(e, ZKE_E_NOMEM, "signature scan: sigs is smaller than the records (zke_sig_scan.sigs_need)");
  for (uint32_t i = 0; i < S.n; i++)
    if (const uint32_t c = o->sig_off[i + 1] - o->sig_off[i]) memcpy(o->sigs + o->sig_off[i], recs + (size_t)i * S.max_sigs, (size_t)c * sizeof(zke_sig_info));
  o->n_sigs = total;
  if (used > S.blob_cap) return fail(e, ZKE_E_NOMEM, "signature scan: sel_blob is smaller than the selectors (zke_sig_scan.sel_blob_need)");
  if (used) memcpy(o->sel_blob, hp + S.blob, used);
  return 0;
}

// A decode from the slot's pinned twin into the caller's zke_keyrec_out: the infos with key_off rewritten to the packed offsets,
// the key bytes compacted (one memcpy per key).  ZKE_E_NOMEM when keys is too small (keys_need says how much).
int deliver_keyrec(zke_engine* e, const KeyrecBufs& b, zke_keyrec_out* o) {
  const KeyrecLayout& K = b.L;
  const uint8_t* hp = b.h_out.as<uint8_t>();
  const zke_key_info* src = reinterpret_cast<const zke_key_info*>(hp);
  size_t total = 0;
  for (uint32_t i = 0; i < K.m; i++) {
    zke_key_info f = src[i];
    if (f.code) f.key_len = 0;
    f.key_off = (uint32_t)total;
    total += f.key_len;
    o->infos[i] = f;
  }
  o->keys_need = total;
  if (total > o->keys_cap) return fail(e, ZKE_E_NOMEM, "key records: keys is smaller than the decoded keys (zke_keyrec_out.keys_need)");
  for (uint32_t i = 0; i < K.m; i++)
    if (o->infos[i].key_len) memcpy(o->keys + o->infos[i].key_off, hp + K.keys + src[i].key_off, o->infos[i].key_len);
  return 0;
}

// A key selection's fold: the records of the (e-mail, candidate) pairs are in the pinned buffer; per e-mail the first ZKE_OK.
void fold_selection(const zke_result* R, const std::vector<uint32_t>& off, zke_result* out, uint32_t* chosen) {
  for (size_t i = 0; i + 1 < off.size(); i++) {
    const uint32_t a = off[i], b = off[i + 1];
    if (a == b) {
      memset(&out[i], 0, sizeof(zke_result));
      out[i].status = ZKE_DKIM_NOT_PASS; out[i].detail = ZKE_D_NEUTRAL;
      chosen[i] = ZKE_SEL_NONE;
      continue;
    }
    uint32_t pick = ZKE_SEL_NONE, flag = 0;
    for (uint32_t k = a; k < b; k++) {
      if (R[k].status == ZKE_OK) { pick = k - a; break; }
      if (R[k].status == ZKE_UNSUPPORTED) flag = ZKE_SEL_AFTER_UNSUPPORTED;
    }
    out[i] = R[pick == ZKE_SEL_NONE ? b - 1 : a + pick];
    chosen[i] = pick == ZKE_SEL_NONE ? ZKE_SEL_NONE : (pick | flag);
  }
}

// `cap_rc` (zke_batch_wait, the synchronous entries): where an extraction's or a scan's shortfall is reported; a slot that retires
// a batch nobody waited for has nobody to tell.
int retire_host(zke_engine* e, Slot& w, int* cap_rc = nullptr) {
  if (w.host_retired == w.host_gen) return 0;
  w.host_retired = w.host_gen;                       // whatever happens below, the batch is no longer pending
  zke_capture_out* pending_caps = w.cap_out;
  w.cap_out = nullptr;
  zke_sig_scan* pending_scan = w.scan_out;
  w.scan_out = nullptr;
  zke_keyrec_out* pending_keyrec = w.keyrec_out;
  w.keyrec_out = nullptr;
  HIPCHK(e, hipEventSynchronize(w.host_done));
  if (w.host_out && w.host_n) memcpy(w.host_out, w.h_results.p, (size_t)w.host_n * sizeof(zke_result));
  w.host_out = nullptr;
  if (!w.sel_off.empty()) {
    fold_selection(w.h_results.as<zke_result>(), w.sel_off, w.sel_out, w.sel_chosen);
    w.sel_off.clear();
  }
  if (pending_scan) {
    const std::string keep = g_err;
    const int r = deliver_scan(e, w.sb, pending_scan);
    if (r == ZKE_E_NOMEM) { if (cap_rc) *cap_rc = r; else g_err = keep; }
    else if (r) return r;
  }
  if (pending_keyrec) {
    const std::string keep = g_err;
    const int r = deliver_keyrec(e, w.kb, pending_keyrec);
    if (r == ZKE_E_NOMEM) { if (cap_rc) *cap_rc = r; else g_err = keep; }
    else if (r) return r;
  }
  if (pending_caps) {
    const std::string keep = g_err;
    const int r = deliver_captures(e, w.cb, pending_caps, w.stream);
    if (r == ZKE_E_NOMEM) { if (cap_rc) *cap_rc = r; else g_err = keep; }
    else if (r) return r;
  }
  return 0;
}

int arg_error(const char* who, const char* what) { g_err = std::string(who) + ": " + what; return ZKE_E_ARG; }
template <class T> bool rising(const T* off, size_t cnt) { uint64_t bad = 0; for (size_t i = 0; i < cnt; i++) bad |= (uint64_t)(off[i + 1] < off[i]); return !bad; }
// The part-id lists of a batch (host arrays in every entry) ...
int check_part_ids(const zke_batch& b, const char* who) {
  return b.with_regex && ((b.n_header_parts && !b.header_part_ids) || (b.n_body_parts && !b.body_part_ids)) ? arg_error(who, "part-id list is null") : 0;
}
// ... and with them the pointers the pipeline reads (device memory; with `host`, the packed host entry's: it also copies the domain
// and key blobs)
int check_batch_pointers(const zke_batch* in, const void* out, bool host, const char* who) {
  if (!in || (in->n && (!out || !in->raw_blob || !in->raw_off || !in->domain_off || !in->key_off || !in->key_type ||
                        (host && (!in->domain_blob || !in->key_blob)))))
    return arg_error(who, "null pointer");
  return check_part_ids(*in, who);
}

// A host batch, checked and measured for the staging image by host_batch(): packed (zke_batch) or gathered (zke_email_ref[n]).
struct HostBatch {
  zke_batch b{};                        // n, the regex section, (packed) the caller's blobs and offsets; capture tables only if any
  const zke_email_ref* refs = nullptr;  // the gathered shape's e-mails (nullptr: packed)
  CaptureReq* cap = nullptr;            // zke_extract_captures: the extraction that rides on this (regex) batch
  const ScanReq* scan = nullptr;        // zke_scan_signatures: sigscan_kernel runs instead of the verify pipeline
  const SelectReq* sel = nullptr;       // zke_select_keys: the batch's entries are (e-mail, candidate key) pairs, folded on delivery
  const KeyrecReq* keyrec = nullptr;    // key records: decoded instead of the verify pipeline, or (with sel) in front of it
  uint64_t raw_total = 0, dom_total = 0, key_total = 0, raw_base = 0, dom_base = 0, key_base = 0;   // blob bytes; off[0] of packed offsets
  size_t cap_words = 0, cap_strs = 0, cap_bytes = 0;      // entries of cap_off and cap_str_off, bytes of cap_blob (0: no tables)
  ImageLayout L{};
};
// Both shapes.  Capture tables: a cap_off whose last entry is 0 holds no string and is no table (cap_str_off, cap_blob unread).
int measure_host_batch(HostBatch& d, const char* who) {
  zke_batch& b = d.b;
  if (d.raw_total > (1ull << 40)) return arg_error(who, "raw e-mails beyond 1 TiB");
  const size_t NP = b.with_regex ? (size_t)b.n * (b.n_header_parts + b.n_body_parts) : 0;
  if (NP && b.cap_off) {
    if (!rising(b.cap_off, NP)) return arg_error(who, "capture offset array is not non-decreasing");
    if (const uint32_t strs = b.cap_off[NP]) {
      if (!b.cap_str_off || !b.cap_blob) return arg_error(who, "capture strings without cap_str_off or cap_blob");
      if (!rising(b.cap_str_off, strs)) return arg_error(who, "capture offset array is not non-decreasing");
      d.cap_words = NP + 1; d.cap_strs = (size_t)strs + 1; d.cap_bytes = b.cap_str_off[strs];
    }
  }
  if (!d.cap_words) b.cap_off = nullptr, b.cap_str_off = nullptr, b.cap_blob = nullptr;
  d.L = image_layout(b.n, d.raw_total, d.dom_total, d.key_total, d.cap_words, d.cap_strs, d.cap_bytes);
  return 0;
}
// The packed shape.  Its offsets are in host memory here, so they are checked (three passes over n + 1 words): a negative length
// would send the staging copy, then the kernels, outside the blobs.  (In device memory they are trusted like the pointers.)
int host_batch(HostBatch& d, const char* who, const zke_result* out, const zke_batch* in) {
  if (int r = check_batch_pointers(in, out, true, who)) return r;
  d = HostBatch{*in};
  if (const uint32_t n = in->n) {
    if (!(rising(in->raw_off, n) && rising(in->domain_off, n) && rising(in->key_off, n))) return arg_error(who, "offset array is not non-decreasing");
    d.raw_base = in->raw_off[0]; d.dom_base = in->domain_off[0]; d.key_base = in->key_off[0];
    d.raw_total = in->raw_off[n] - d.raw_base; d.dom_total = in->domain_off[n] - d.dom_base; d.key_total = in->key_off[n] - d.key_base;
  }
  return measure_host_batch(d, who);
}
// The gathered shape: the e-mails one by one, lists == nullptr for verify_email.
int host_batch(HostBatch& d, const char* who, const zke_result* out, const zke_email_ref* refs, uint32_t n, const zke_regex_lists* lists) {
  if (n && (!refs || !out)) return arg_error(who, "null pointer");
  d = HostBatch{zke_batch{n}, refs};
  if (lists) {
    d.b.with_regex = 1; d.b.n_header_parts = lists->n_header_parts; d.b.header_part_ids = lists->header_part_ids;
    d.b.n_body_parts = lists->n_body_parts; d.b.body_part_ids = lists->body_part_ids;
    d.b.cap_off = lists->cap_off; d.b.cap_str_off = lists->cap_str_off; d.b.cap_blob = lists->cap_blob;
  }
  if (int r = check_part_ids(d.b, who)) return r;
  for (uint32_t i = 0; i < n; i++) {
    const zke_email_ref& m = refs[i];
    if ((m.raw_len && !m.raw) || (m.domain_len && !m.from_domain) || (m.key_len && !m.key)) return arg_error(who, "null buffer with a length");
    if (m.raw_len > (1ull << 40) || m.domain_len > (1ull << 32) || m.key_len > (1ull << 32)) return arg_error(who, "implausible length");
    d.raw_total += m.raw_len; d.dom_total += m.domain_len; d.key_total += m.key_len;
  }
  return measure_host_batch(d, who);
}

// One host batch into slot w (caller holds its lock): pack -> one H2D -> the launches -> one D2H -> event.
int submit_host(zke_engine* e, Slot& w, const HostBatch& d, zke_result* out, bool want_em, bool want_clean) {
  const uint32_t n = d.b.n;
  const ImageLayout& L = d.L;
  if (int r = retire_host(e, w)) return r;           // the pinned buffers are about to be overwritten
  if (int r = ensure_host_buffers(e, w, L.total, n)) return r;      // (a no-op: submit_host_batch has grown every slot's staging)
  if (d.cap) {
    if (int r = ensure_capture_buffers(e, w.cb, n, d.cap->P, d.cap->G, d.cap->out->cap_blob_cap, d.cap->needs_work)) return r;
    w.cb.L = cap_layout(n, d.cap->P, d.cap->G, d.cap->out->cap_blob_cap);
  }
  if (d.scan) {      // (a selector is at most ZKE_MAX_TAGBUF bytes: a larger blob than that per record slot is never used)
    const size_t blob = std::min<size_t>(d.scan->out->sel_blob_cap, (size_t)n * d.scan->max_sigs * ZKE_MAX_TAGBUF);
    if (int r = ensure_scan_buffers(e, w.sb, n, d.scan->max_sigs, blob)) return r;
  }
  if (d.keyrec)
    if (int r = ensure_keyrec_buffers(e, w.kb, n, (size_t)(d.sel ? d.key_total : d.raw_total), d.sel != nullptr)) return r;
  uint8_t* hp = w.h_image.as<uint8_t>();
  if (d.refs) {
    // the CSR arrays are written where they will be read from (prefix sums over the lengths), and every e-mail's three buffers
    // go to their places in the blobs — the pool takes runs of consecutive e-mails (CopyPool::gather)
    uint64_t* ro = reinterpret_cast<uint64_t*>(hp + L.raw_off), *dofs = reinterpret_cast<uint64_t*>(hp + L.dom_off), *ko = reinterpret_cast<uint64_t*>(hp + L.key_off);
    uint8_t* kt = hp + L.key_type, *xn = hp + L.ext_null;
    w.gather.resize((size_t)3 * n);
    uint64_t r = 0, dd = 0, k = 0;
    for (uint32_t i = 0; i < n; i++) {
      const zke_email_ref& m = d.refs[i];
      ro[i] = r; dofs[i] = dd; ko[i] = k;
      kt[i] = (uint8_t)(m.key_type > ZKE_KEY_OTHER ? ZKE_KEY_OTHER : m.key_type);
      xn[i] = m.external_input_null ? 1 : 0;
      w.gather[i] = CopyPool::Piece{hp + L.raw + r, m.raw, m.raw_len};                       // three runs, each contiguous in the image
      w.gather[(size_t)n + i] = CopyPool::Piece{hp + L.dom + dd, m.from_domain, m.domain_len};
      w.gather[2 * (size_t)n + i] = CopyPool::Piece{hp + L.key + k, m.key, m.key_len};
      r += m.raw_len; dd += m.domain_len; k += m.key_len;
    }
    ro[n] = r; dofs[n] = dd; ko[n] = k;
    if (e->pool) e->pool->gather(w.gather.data(), w.gather.size());
    else for (const auto& p : w.gather) if (p.n) stage_copy(p.dst, p.src, p.n, ZKE_GATHER_STREAM_FROM);
  } else {
    // the offsets are copied as they are (the kernels subtract off[0] themselves and the device pointers below are biased
    // by -off[0]): nothing is rebased, nothing is allocated, every byte is written once
    CopyPool::Piece pc[8] = {
        {hp + L.raw_off, d.b.raw_off, (size_t)(n + 1) * 8}, {hp + L.dom_off, d.b.domain_off, (size_t)(n + 1) * 8},
        {hp + L.key_off, d.b.key_off, (size_t)(n + 1) * 8}, {hp + L.key_type, d.b.key_type, n},
        {hp + L.ext_null, d.b.ext_null, d.b.ext_null ? n : 0u}, {hp + L.raw, d.b.raw_blob + d.raw_base, (size_t)d.raw_total},
        {hp + L.dom, d.b.domain_blob + d.dom_base, (size_t)d.dom_total}, {hp + L.key, d.b.key_blob + d.key_base, (size_t)d.key_total}};
    if (e->pool) e->pool->copy(pc, 8);
    else for (const auto& p : pc) if (p.n) stage_copy(p.dst, p.src, p.n);
  }
  if (d.cap_words) {       // the capture tables of a regex batch (small)
    stage_copy(hp + L.cap_off, d.b.cap_off, d.cap_words * 4);
    stage_copy(hp + L.cap_str_off, d.b.cap_str_off, d.cap_strs * 4);
    stage_copy(hp + L.cap_blob, d.b.cap_blob, d.cap_bytes);
  }
  hipStream_t s = w.stream;
  SlotUse use(e, w, s);
  if (int r = use.acquire()) return r;
  StageTimer tm(e, &w, s);
  tm.mark(MK_START);
#ifndef ZKE_HOST_COPY_STREAM
#define ZKE_HOST_COPY_STREAM 1
#endif
  if (ZKE_HOST_COPY_STREAM && L.total >= (256u << 10)) {
    // The image crosses PCIe on one of the engine's TWO copy streams, taken in turn, and the slot's stream waits for it.  Issued
    // on the slots' own 22 streams the input copies moved 31 GB/s in aggregate — one DMA engine's rate —, on one copy stream the
    // same; on two, 48 GB/s = 84 % of the link (122 us per 1 024-e-mail batch instead of 186; three streams: 141 us, four: worse).
    // Nothing on the device has to be waited for first: the slot's previous host batch — the only earlier user of d_image — was
    // retired on the host before the image was packed.  (Small images stay on the slot's stream: the cross-stream event costs a
    // single e-mail 16 us of latency and buys nothing.)
    std::lock_guard<std::mutex> cg(e->copy_mu);
    hipStream_t cs = e->copy_stream[e->copy_turn++ % ZKE_COPY_STREAMS];
    HIPCHK(e, hipMemcpyAsync(w.d_image.p, hp, L.total, hipMemcpyHostToDevice, cs));
    HIPCHK(e, hipEventRecord(w.h2d_done, cs));
    HIPCHK(e, hipStreamWaitEvent(s, w.h2d_done, 0));
  } else {
    HIPCHK(e, hipMemcpyAsync(w.d_image.p, hp, L.total, hipMemcpyHostToDevice, s));
  }
  tm.mark(MK_H2D);
  uint8_t* dp = w.d_image.as<uint8_t>();
  zke_batch dv = d.b;
  dv.raw_off = reinterpret_cast<const uint64_t*>(dp + L.raw_off);
  dv.domain_off = reinterpret_cast<const uint64_t*>(dp + L.dom_off);
  dv.key_off = reinterpret_cast<const uint64_t*>(dp + L.key_off);
  dv.raw_blob = dp + L.raw - d.raw_base;
  dv.domain_blob = dp + L.dom - d.dom_base;
  dv.key_blob = dp + L.key - d.key_base;
  dv.key_type = dp + L.key_type;
  dv.ext_null = (d.refs || d.b.ext_null) ? dp + L.ext_null : nullptr;
  dv.cap_off = d.cap_words ? reinterpret_cast<const uint32_t*>(dp + L.cap_off) : nullptr;
  dv.cap_str_off = d.cap_words ? reinterpret_cast<const uint32_t*>(dp + L.cap_str_off) : nullptr;
  dv.cap_blob = d.cap_words ? dp + L.cap_blob : nullptr;
  if (d.scan) {
    // one launch, no verify workspace: the counter of selector bytes starts at zero, everything comes back as one copy
    const ScanLayout& S = w.sb.L;
    uint8_t* so = w.sb.out.as<uint8_t>();
    HIPCHK(e, hipMemsetAsync(so, 0, 64, s));
    SigScanArgs sa{};
    sa.n = n; sa.max_sigs = S.max_sigs;
    sa.raw = dv.raw_blob; sa.raw_off = dv.raw_off; sa.dom = dv.domain_blob; sa.dom_off = dv.domain_off;
    sa.strict = e->strict; sa.now = batch_clock(e);
    sa.status = reinterpret_cast<uint32_t*>(so + S.status);
    sa.recs = reinterpret_cast<zke_sig_info*>(so + S.recs);
    sa.sel_blob = so + S.blob; sa.sel_cap = (uint32_t)S.blob_cap;
    sa.sel_used = reinterpret_cast<uint32_t*>(so);
    sa.hdr_ovf = w.sb.ovf.as<uint32_t>();
    hipLaunchKernelGGL(sigscan_kernel, dim3(n), dim3(64), 0, s, sa);
    HIPCHK(e, hipGetLastError());
    tm.mark(MK_FRONT); tm.mark(MK_HASH); tm.mark(MK_VERDICT);      // zke_timings.front_end_us is the scan; the other stages are empty
    HIPCHK(e, hipMemcpyAsync(w.sb.h_out.p, so, S.total, hipMemcpyDeviceToHost, s));
  } else if (d.keyrec && !d.sel) {
    // one launch over the records (the image's raw section), infos and keys back as one copy
    const KeyrecLayout& K = w.kb.L;
    uint8_t* ko = w.kb.out.as<uint8_t>();
    const KeyrecArgs ka{n, d.keyrec->mode, dv.raw_blob, dv.raw_off, reinterpret_cast<zke_key_info*>(ko), ko + K.keys};
    hipLaunchKernelGGL(keyrec_kernel, dim3(n), dim3(64), 0, s, ka);
    HIPCHK(e, hipGetLastError());
    tm.mark(MK_FRONT); tm.mark(MK_HASH); tm.mark(MK_VERDICT);      // zke_timings.front_end_us is the decode; the other stages are empty
    HIPCHK(e, hipMemcpyAsync(w.kb.h_out.p, ko, K.total, hipMemcpyDeviceToHost, s));
  } else {
  uint64_t key_hint = d.key_total;
  if (d.keyrec) {
    // the image's key section holds the candidates' RECORDS: decode them, then scan the lengths and gather the keys into the
    // packed CSR the front end reads — three small launches, the keys never leave HBM
    const KeyrecLayout& K = w.kb.L;
    uint8_t* ko = w.kb.out.as<uint8_t>();
    uint8_t* pk = w.kb.pack.as<uint8_t>();
    const KeyrecArgs ka{n, d.keyrec->mode, dv.key_blob, dv.key_off, reinterpret_cast<zke_key_info*>(ko), ko + K.keys};
    hipLaunchKernelGGL(keyrec_kernel, dim3(n), dim3(64), 0, s, ka);
    const KeyrecPackArgs pa{n, ka.infos, ka.keys, reinterpret_cast<uint64_t*>(pk), pk + K.p_type, pk + K.p_blob};
    hipLaunchKernelGGL(keyrec_pack_kernel, dim3(1), dim3(64), 0, s, pa);
    hipLaunchKernelGGL(keyrec_gather_kernel, dim3(n), dim3(64), 0, s, pa);
    HIPCHK(e, hipGetLastError());
    dv.key_blob = pa.key_blob; dv.key_off = pa.key_off; dv.key_type = pa.key_type;
    // (run_device_pipeline reads "the keys average more than an RSA-2048 key's 270 bytes" from the total: a 2048-bit
    // SubjectPublicKeyInfo record is about 410 characters, a 3072-bit one 580)
    key_hint = d.key_total > (uint64_t)n * 480 ? (uint64_t)n * 273 : 0;
  }
  if (int r = run_device_pipeline(e, w, &dv, d.raw_total, key_hint, w.d_results.as<zke_result>(), s, want_em, batch_clock(e), want_clean, d.cap)) return r;
  HIPCHK(e, hipMemcpyAsync(w.h_results.p, w.d_results.p, (size_t)n * sizeof(zke_result), hipMemcpyDeviceToHost, s));
  if (d.keyrec) HIPCHK(e, hipMemcpyAsync(w.kb.h_out.p, w.kb.out.p, w.kb.L.total, hipMemcpyDeviceToHost, s));
  }
  if (d.cap) HIPCHK(e, hipMemcpyAsync(w.cb.h_cap.p, w.cb.cap.p, w.cb.L.fixed_end, hipMemcpyDeviceToHost, s));
  tm.mark(MK_D2H);
  HIPCHK(e, hipEventRecord(w.host_done, s));
  w.host_gen++;
  w.host_out = (d.scan || d.sel || d.keyrec) ? nullptr : out; w.host_n = n;
  w.keyrec_out = d.keyrec ? d.keyrec->out : nullptr;
  w.cap_out = d.cap ? d.cap->out : nullptr;
  w.scan_out = d.scan ? d.scan->out : nullptr;
  w.sel_off.clear();
  if (d.sel) {
    w.sel_off.resize((size_t)d.sel->n + 1);
    for (uint32_t i = 0; i <= d.sel->n; i++) w.sel_off[i] = d.sel->cand_off[i] - d.sel->cand_off[0];
    w.sel_out = d.sel->out; w.sel_chosen = d.sel->chosen;
  }
  return use.release();
}

// The host entry's staging of EVERY slot, sized for images of `image` bytes and n records.  Pinned memory that comes into being
// while other slots' copies are in flight copies at a fraction of the link's rate for the rest of its life (measured: slots that
// allocated their staging lazily, one by one under traffic, moved 9 GB/s in aggregate; the same buffers allocated together in a
// quiet moment 31 GB/s) — so growth is a stop-the-world event: no submission in progress (`big` exclusive), every pending host
// batch delivered, every stream drained, then all slots at once, with headroom so that it stays rare.
int grow_host_staging(zke_engine* e, size_t image, uint32_t n) {
  std::unique_lock<std::shared_mutex> ex(e->big);
  if (image <= e->host_image_cap.load() && n <= e->host_n_cap.load()) return 0;       // another thread grew it meanwhile
  HIPCHK(e, hipSetDevice(e->device));
  for (Slot* w : e->slots) { std::lock_guard<std::mutex> g(w->mu); if (int r = retire_host(e, *w)) return r; }
  if (int r = drain_engine(e, false)) return r;
  for (auto& cs : e->copy_stream)
    if (!cs) HIPCHK(e, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  const size_t want_image = std::max(image + image / 2, e->host_image_cap.load());
  const uint32_t want_n = std::max<uint32_t>(n + n / 2, e->host_n_cap.load());
  for (Slot* w : e->slots)
    if (int r = ensure_host_buffers(e, *w, want_image, want_n)) return r;
  e->host_image_cap = want_image;
  e->host_n_cap = want_n;
  return 0;
}
// Parity intermediates (tests) of the packed batch `in` just delivered from slot w: its scratch copied back, sliced on the host.
int copy_debug_out(zke_engine* e, Slot& w, const zke_batch& in, const zke_result* out, const zke_debug_out* dbg) {
  const uint32_t n = in.n;
  const uint64_t raw_total = in.raw_off[n] - in.raw_off[0];
  std::vector<EmailMeta> meta(n), meta2;
  HIPCHK(e, hipMemcpy(meta.data(), w.meta.p, (size_t)n * sizeof(EmailMeta), hipMemcpyDeviceToHost));
  const size_t scratch_bytes = 2 * (size_t)raw_total + (size_t)(n + 1) * SCR_PER_EMAIL + 256;
  std::vector<uint8_t> scr(scratch_bytes);
  HIPCHK(e, hipMemcpy(scr.data(), w.scratch.p, scratch_bytes, hipMemcpyDeviceToHost));
  std::vector<uint8_t> em, clean;
  if (dbg->em) { em.resize((size_t)n * 512); HIPCHK(e, hipMemcpy(em.data(), w.em_dbg.p, em.size(), hipMemcpyDeviceToHost)); }
  if (dbg->clean_body && in.with_regex) {
    meta2.resize(n);
    HIPCHK(e, hipMemcpy(meta2.data(), w.meta2.p, (size_t)n * sizeof(EmailMeta), hipMemcpyDeviceToHost));
    clean.resize((size_t)raw_total + (size_t)(n + 1) * CLEAN_PER_EMAIL + 256);
    HIPCHK(e, hipMemcpy(clean.data(), w.clean.p, clean.size(), hipMemcpyDeviceToHost));
  }
  auto put = [](uint8_t* base, size_t stride, uint32_t i, const uint8_t* src, size_t len) {
    if (!base) return;
    memset(base + (size_t)i * stride, 0, stride);
    memcpy(base + (size_t)i * stride, src, std::min(len, stride));
  };
  for (uint32_t i = 0; i < n; i++) {
    const EmailMeta& m = meta[i];
    const uint64_t rel = in.raw_off[i] - in.raw_off[0];
    const uint32_t raw_len = (uint32_t)(in.raw_off[i + 1] - in.raw_off[i]);
    const uint8_t* regA = scr.data() + host_scratch_off(in.raw_off, i);
    const uint8_t* regB = regA + (((size_t)raw_len + PRE_SLACK + 15) & ~(size_t)15);
    const bool hashed = out[i].canon_header_len || out[i].canon_body_len || m.canon_full_len;
    put(dbg->canon_header, dbg->canon_header_stride, i, regA, hashed ? out[i].canon_header_len : 0);
    const uint8_t* body = m.body_src_is_raw ? in.raw_blob + in.raw_off[i] + m.body_off : regB;
    put(dbg->canon_body, dbg->canon_body_stride, i, body, hashed ? m.canon_full_len : 0);
    if (dbg->canon_body_full_len) dbg->canon_body_full_len[i] = hashed ? m.canon_full_len : 0;
    if (dbg->rsa_route) dbg->rsa_route[i] = m.rsa_route;
    if (dbg->em) put(dbg->em, dbg->em_stride, i, em.data() + (size_t)i * 512 + 512 - std::min<uint32_t>(512, e_k(out[i].rsa_bits)),
                     std::min<uint32_t>(512, e_k(out[i].rsa_bits)));
    if (dbg->clean_body && in.with_regex && meta2[i].state == ST_CAND)
      put(dbg->clean_body, dbg->clean_body_stride, i, clean.data() + (rel + (uint64_t)i * CLEAN_PER_EMAIL), meta2[i].hashed_len);
    else if (dbg->clean_body)
      put(dbg->clean_body, dbg->clean_body_stride, i, nullptr, 0);
  }
  return 0;
}

// Every host entry's submission.  With a ticket: asynchronous (zke_batch_wait or the slot's next batch delivers).  Without: delivered
// before this returns, the parity intermediates (dbg) copied back under the same slot lock — the slot's next batch overwrites them.
int submit_host_batch(zke_engine* e, const HostBatch& d, zke_result* out, uint64_t* ticket, const zke_debug_out* dbg = nullptr) {
  const uint32_t n = d.b.n;
  if (!n && !ticket) return 0;
  if (n && (d.L.total > e->host_image_cap.load() || n > e->host_n_cap.load())) if (int r = grow_host_staging(e, d.L.total, n)) return r;
  std::shared_lock<std::shared_mutex> sh(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  if (d.cap) capture_resolve(e, *d.cap);             // under `big`: the programs' tables cannot be freed before the batch is enqueued
  uint32_t slot;
  Slot& w = next_slot(e, slot);
  std::lock_guard<std::mutex> g(w.mu);
  if (!n) { *ticket = make_ticket(slot, w.host_retired); return 0; }      // nothing to wait for
  if (int r = submit_host(e, w, d, out, dbg && dbg->em, dbg && dbg->clean_body)) return r;
  if (ticket) { *ticket = make_ticket(slot, w.host_gen); return 0; }
  int cap_rc = 0;
  if (int r = retire_host(e, w, &cap_rc)) return r;
  if (cap_rc) return cap_rc;
  return dbg ? copy_debug_out(e, w, d.b, out, dbg) : 0;
}

// ---- the DFA registry (dfa_registry.hip.h has the blob parser and the entry type)
// (caller holds reg_mu exclusively, and the engine is idle or the entry was never handed out)
void drop_dfa(zke_engine* e, uint32_t id) {
  RegisteredDfa* d = e->dfas[id];
  auto range = e->dfa_index.equal_range(d->hash);
  for (auto it = range.first; it != range.second; ++it)
    if (it->second == id) { e->dfa_index.erase(it); break; }
  d->blob.release(); d->dev.release();
  delete d;
  e->dfas[id] = nullptr;
  e->dfa_live--;
}

// (caller holds reg_mu, shared or exclusive)
bool dfa_lookup(zke_engine* e, uint64_t h, const uint8_t* fwd, size_t fl, const uint8_t* bwd, size_t bl, uint32_t* id, bool pin) {
  auto range = e->dfa_index.equal_range(h);
  for (auto it = range.first; it != range.second; ++it) {
    RegisteredDfa* d = e->dfas[it->second];
    if (d && d->fwd_copy.size() == fl && d->bwd_copy.size() == bl && (!fl || !memcmp(d->fwd_copy.data(), fwd, fl)) &&
        (!bl || !memcmp(d->bwd_copy.data(), bwd, bl))) {
      d->last_use.store(e->reg_clock.fetch_add(1) + 1, std::memory_order_relaxed);
      if (pin) d->pins.fetch_add(1);
      *id = it->second;
      return true;
    }
  }
  return false;
}

// The registry is full: drop the least recently used pair among those zke_verify_email_with_regex registered on its own.
// The tables may be in use by batches in flight, so the engine is drained first (exclusive lock + stream syncs).
int dfa_evict_one(zke_engine* e) {
  std::unique_lock<std::shared_mutex> ex(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  if (int r = drain_engine(e, false)) return r;
  std::unique_lock<std::shared_mutex> rl(e->reg_mu);
  uint32_t victim = 0xFFFFFFFFu;
  uint64_t oldest = ~0ull;
  for (uint32_t k = 0; k < e->dfas.size(); k++) {
    const RegisteredDfa* d = e->dfas[k];
    if (d && d->transient && !d->pins.load() && d->last_use.load(std::memory_order_relaxed) < oldest) { oldest = d->last_use.load(std::memory_order_relaxed); victim = k; }
  }
  if (victim == 0xFFFFFFFFu) return fail(e, ZKE_E_NOMEM, "DFA registry full (zke_options.max_dfas): zke_dfa_unregister pairs no longer needed (pairs of per-e-mail calls in progress cannot be evicted)");
  drop_dfa(e, victim);
  return 0;
}

// transient: registered by a per-e-mail call on its own — evictable, and PINNED for the caller (dfa_unpin when its batch is done)
int dfa_register_impl(zke_engine* e, const uint8_t* fwd, size_t fwd_len, const uint8_t* bwd, size_t bwd_len, uint32_t* out_id, bool transient) {
  if (!e || !out_id || (fwd_len && !fwd) || (bwd_len && !bwd)) return ZKE_E_ARG;
  const uint64_t h = pair_hash(fwd, fwd_len, bwd, bwd_len);
  {
    // registering the same pair again returns the id it already has (per-e-mail callers re-submit their part list)
    std::shared_lock<std::shared_mutex> rl(e->reg_mu);
    if (dfa_lookup(e, h, fwd, fwd_len, bwd, bwd_len, out_id, transient)) return 0;
  }
  HIPCHK(e, hipSetDevice(e->device));
  RegisteredDfa* rd = new RegisteredDfa();
  auto discard = [&]() { rd->blob.release(); rd->dev.release(); delete rd; };
  rd->fwd_copy.assign(fwd, fwd + fwd_len);
  rd->bwd_copy.assign(bwd, bwd + bwd_len);
  rd->hash = h;
  rd->transient = transient;
  {
    HostDfa hf, hr;
    uint32_t det = parse_dfa_blob(fwd, fwd_len, hf);
    if (!det) { det = parse_dfa_blob(bwd, bwd_len, hr); if (det) det += ZKE_D_DFA_BWD_OFFSET; }
    rd->detail = det;
    rd->valid = det == 0;
    if (rd->valid) {
      auto packed = [](const HostDfa& x) { return (((size_t)x.d.table_len * (x.d.wide ? 4 : 2)) + 15) & ~(size_t)15; };
      const size_t fb = packed(hf), rb = packed(hr);
      rd->lds_bytes = fb + rb;
      rd->idle = dfa_idle_state(hf);
      int r = 0;
      if ((r = rd->blob.ensure(fb + rb + 64)) || (r = rd->dev.ensure(sizeof(RegexDev)))) { discard(); return fail(e, r, "hipMalloc"); }
      std::vector<uint8_t> img(fb + rb + 64, 0);
      auto pack = [&](const HostDfa& x, size_t off) {
        if (x.d.wide) memcpy(img.data() + off, x.table.data(), x.table.size() * 4);
        else { uint16_t* o = reinterpret_cast<uint16_t*>(img.data() + off); for (size_t i = 0; i < x.table.size(); i++) o[i] = (uint16_t)x.table[i]; }
      };
      pack(hf, 0); pack(hr, fb);
      RegexDev rdv{};
      rdv.fwd = hf.d; rdv.rev = hr.d;
      rdv.fwd.table = (uint64_t)rd->blob.as<uint8_t>();
      rdv.rev.table = (uint64_t)(rd->blob.as<uint8_t>() + fb);
      hipError_t he = hipMemcpy(rd->blob.p, img.data(), img.size(), hipMemcpyHostToDevice);
      if (he == hipSuccess) he = hipMemcpy(rd->dev.p, &rdv, sizeof rdv, hipMemcpyHostToDevice);
      if (he != hipSuccess) { discard(); return fail(e, ZKE_E_DEVICE, "dfa upload", he); }
    }
  }
  for (;;) {
    {
      std::unique_lock<std::shared_mutex> rl(e->reg_mu);
      if (dfa_lookup(e, h, fwd, fwd_len, bwd, bwd_len, out_id, transient)) { discard(); return 0; }      // another thread was first
      if (e->dfa_live < e->opt.max_dfas) {
        if (rd->valid && rd->lds_bytes + 1024 <= 150 * 1024)       // the tables fit in LDS: the DFA kernels are launched with that much
          if (int r = raise_dfa_lds_attrs(e, rd->lds_bytes + 1024)) { discard(); return r; }
        uint32_t id = 0;
        while (id < e->dfas.size() && e->dfas[id]) id++;
        if (id == e->dfas.size()) e->dfas.push_back(nullptr);
        rd->last_use.store(e->reg_clock.fetch_add(1) + 1, std::memory_order_relaxed);
        rd->pins.store(transient ? 1u : 0u);
        e->dfas[id] = rd;
        e->dfa_index.emplace(h, id);
        e->dfa_live++;
        *out_id = id;
        return 0;
      }
    }
    if (int r = dfa_evict_one(e)) { discard(); return r; }
  }
}

void dfa_unpin(zke_engine* e, const std::vector<uint32_t>& ids) {
  std::shared_lock<std::shared_mutex> rl(e->reg_mu);
  for (uint32_t id : ids) e->dfas[id]->pins.fetch_sub(1);          // (a pinned entry is neither evicted nor unregistered: it is there)
}

}  // namespace

extern "C" {

int zke_dfa_register(zke_engine* e, const uint8_t* fwd, size_t fwd_len, const uint8_t* bwd, size_t bwd_len, uint32_t* out_id) {
  return dfa_register_impl(e, fwd, fwd_len, bwd, bwd_len, out_id, false);
}

int zke_dfa_status(zke_engine* e, uint32_t id, uint32_t* detail) {
  if (!e || !detail) return ZKE_E_ARG;
  std::shared_lock<std::shared_mutex> rl(e->reg_mu);
  if (id >= e->dfas.size() || !e->dfas[id]) return fail(e, ZKE_E_DFA, "zke_dfa_status: id is not registered");
  *detail = e->dfas[id]->detail;
  return 0;
}

int zke_dfa_unregister(zke_engine* e, uint32_t id) {
  if (!e) return ZKE_E_ARG;
  std::unique_lock<std::shared_mutex> ex(e->big);         // no submission in progress ...
  HIPCHK(e, hipSetDevice(e->device));
  if (int r = drain_engine(e, false)) return r;           // ... and nothing in flight that could still read the tables
  std::unique_lock<std::shared_mutex> rl(e->reg_mu);
  if (id >= e->dfas.size() || !e->dfas[id]) return fail(e, ZKE_E_DFA, "zke_dfa_unregister: id is not registered");
  if (e->dfas[id]->pins.load()) return fail(e, ZKE_E_DFA, "zke_dfa_unregister: a zke_verify_email_with_regex call in progress uses this pair");
  drop_dfa(e, id);
  return 0;
}

int zke_engine_reserve(zke_engine* e, uint32_t max_n, uint64_t max_raw_total, uint32_t slots, uint32_t max_regex_parts) {
  if (!e || slots == 0 || slots > 64) return ZKE_E_ARG;
  std::unique_lock<std::shared_mutex> ex(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  while (e->slots.size() < slots) {
    Slot* w = new_slot(e);
    if (!w) return ZKE_E_DEVICE;
    e->slots.push_back(w);
  }
  if (max_n)
    for (Slot* w : e->slots)
      if (int r = ensure_workspace(e, *w, max_n, max_raw_total, max_regex_parts != 0, max_regex_parts, false)) return r;
  if (max_n && max_regex_parts)          // the capture workspace: four groups of 32 bytes per part is what a larger extraction regrows from
    for (Slot* w : e->slots)
      if (int r = ensure_capture_buffers(e, w->cb, max_n, max_regex_parts, 4 * max_regex_parts, (size_t)max_n * max_regex_parts * 128, true)) return r;

  // A stream's hardware queue and the queue's scratch memory (the front end spills a few registers) come into being
  // with the first launch that needs them — milliseconds, and they would land in the first batch of every slot.
  // One trivial launch per slot, with more scratch per lane than any kernel of the pipeline, pays for both here.
  // Then one empty e-mail through the whole pipeline of every slot: kernel code, kernel arguments and the slot's workspace
  // pages have all been touched once before the first real batch arrives.
  if (int r = e->misc.ensure(1024)) return fail(e, r, "workspace allocation");
  HIPCHK(e, hipMemset(e->misc.p, 0, 1024));
  zke_batch wb{};
  wb.n = 1;
  uint8_t* z = e->misc.as<uint8_t>();            // 1 KB of zeros: CSR offsets {0, 0}, empty blobs, key type "rsa"
  wb.raw_blob = z + 512; wb.raw_off = reinterpret_cast<const uint64_t*>(z);
  wb.domain_blob = z + 512; wb.domain_off = reinterpret_cast<const uint64_t*>(z);
  wb.key_blob = z + 512; wb.key_off = reinterpret_cast<const uint64_t*>(z);
  wb.key_type = z + 512; wb.ext_null = nullptr;
  const bool timing = e->timing.exchange(false);
  for (Slot* w : e->slots) {
    hipLaunchKernelGGL(slot_warm_kernel, dim3(1), dim3(64), 0, w->stream, (uint32_t*)nullptr);
    if (max_n) {
      SlotUse use(e, *w, w->stream);
      int r = use.acquire();
      if (!r) r = run_device_pipeline(e, *w, &wb, 0, 0, reinterpret_cast<zke_result*>(z + 768), w->stream, false, 0);
      if (r) { e->timing = timing; return r; }
      (void)use.release();
    }
  }
  e->timing = timing;
  HIPCHK(e, hipGetLastError());
  for (Slot* w : e->slots) HIPCHK(e, hipStreamSynchronize(w->stream));
  if (e->host_image_cap.load())          // slots created just now get the staging the others have (everything is drained: see grow_host_staging)
    for (Slot* w : e->slots)
      if (int r = ensure_host_buffers(e, *w, e->host_image_cap.load(), e->host_n_cap.load())) return r;
  return 0;
}

int zke_engine_reserve_host(zke_engine* e, uint32_t max_n, uint64_t max_input_bytes) {
  if (!e) return ZKE_E_ARG;
  // offsets, key types and 64-byte alignment on top of the blobs (image_layout)
  const size_t image = (size_t)max_input_bytes + (size_t)(max_n + 1) * 24 + 2 * (size_t)max_n + 16 * 64 + 4 * 64;
  if (image <= e->host_image_cap.load() && max_n <= e->host_n_cap.load()) return 0;
  return grow_host_staging(e, image, max_n);
}

int zke_verify_batch_device(zke_engine* e, const zke_batch* in, uint64_t raw_total, uint64_t domain_total, uint64_t key_total,
                            zke_result* out_dev, void* stream) {
  (void)domain_total;
  if (!e) return ZKE_E_ARG;
  if (int r = check_batch_pointers(in, out_dev, false, "zke_verify_batch_device")) return r;
  std::shared_lock<std::shared_mutex> sh(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  // Submission slots are taken round-robin: with S slots, S batches are in flight before a workspace is reused.
  uint32_t slot;
  Slot& w = next_slot(e, slot);
  std::lock_guard<std::mutex> g(w.mu);
  hipStream_t s = stream ? (hipStream_t)stream : w.stream;
  const uint64_t now = batch_clock(e);
  SlotUse use(e, w, s);
  if (int r = use.acquire()) return r;
  const bool graphs = e->opt.replay_graphs && !e->timing.load() && !((e->strict & ZKE_STRICT_EXPIRY_X) && !e->opt.now_unix);
  if (!graphs) {
    // Launched eagerly: three kernels per signature round (front end, hash / modexp stage, Ed25519 + verdict)
    if (int r = run_device_pipeline(e, w, in, raw_total, key_total, out_dev, s, false, now)) return r;
    return use.release();
  }
  // hipGraph replay (opt-in).  A service re-submits batches that live in the same staging buffers: the second time a
  // slot sees a descriptor byte for byte — input pointers and sizes, output pointer, part ids, rounds, key-size hint —
  // its kernel sequence is captured, and replayed from then on.  The key also holds the slot's workspace generation: a
  // graph bakes in the workspace pointers, and a batch that regrew a buffer in between (DevBuf::ensure frees and
  // reallocates) would leave them dangling.  Nothing in the submit path calls hipMalloc / hipFuncSetAttribute once the
  // workspaces are reserved, so the capture contains kernel nodes only.
  const uint32_t nh = in->with_regex ? in->n_header_parts : 0, nb = in->with_regex ? in->n_body_parts : 0;
  std::vector<uint8_t> key(sizeof(zke_batch) + 5 * sizeof(uint64_t) + 4 * (size_t)(nh + nb));
  {
    zke_batch kb = *in;
    kb.header_part_ids = nullptr; kb.body_part_ids = nullptr;          // host arrays: compared by content below
    uint8_t* p = key.data();
    memset(p, 0, key.size());
    memcpy(p, &kb.n, sizeof kb.n);                                     // field by field: the struct's padding is not copied
    size_t o = 8;
    const void* ptrs[] = {kb.raw_blob, kb.raw_off, kb.domain_blob, kb.domain_off, kb.key_blob, kb.key_off, kb.key_type, kb.ext_null,
                          kb.cap_off, kb.cap_str_off, kb.cap_blob, out_dev, s};
    for (const void* q : ptrs) { memcpy(p + o, &q, sizeof q); o += sizeof q; }
    const uint64_t nums[] = {raw_total, key_total, ((uint64_t)kb.with_regex << 32) | e->opt.max_sig_rounds, ((uint64_t)kb.n_header_parts << 32) | kb.n_body_parts,
                             w.generation};
    (void)o;
    uint8_t* tail = p + sizeof(zke_batch);
    memcpy(tail, nums, sizeof nums);
    tail += sizeof nums;
    if (nh) memcpy(tail, in->header_part_ids, 4 * (size_t)nh);
    tail += 4 * (size_t)nh;
    if (nb) memcpy(tail, in->body_part_ids, 4 * (size_t)nb);
  }
  static_assert(8 + 13 * sizeof(void*) <= sizeof(zke_batch), "graph key layout");
  if (w.graph_exec && key == w.graph_key) {
    HIPCHK(e, hipGraphLaunch(w.graph_exec, s));
    return use.release();
  }
  if (w.graph_exec) { (void)hipGraphExecDestroy(w.graph_exec); w.graph_exec = nullptr; }
  if (key != w.graph_key) {               // first sighting: run eagerly (this is also what sizes the workspaces)
    if (int r = run_device_pipeline(e, w, in, raw_total, key_total, out_dev, s, false, now)) return r;
    // the generation may have moved: remember the key as it is now, so that an identical second call captures
    const uint64_t gen = w.generation;
    memcpy(key.data() + sizeof(zke_batch) + 4 * sizeof(uint64_t), &gen, sizeof gen);
    w.graph_key = key;
    return use.release();
  }
  hipGraph_t g2 = nullptr;
  HIPCHK(e, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  const int r = run_device_pipeline(e, w, in, raw_total, key_total, out_dev, s, false, now);
  const hipError_t ce = hipStreamEndCapture(s, &g2);
  hipGraphExec_t ge = nullptr;
  if (!r && ce == hipSuccess && g2 && hipGraphInstantiate(&ge, g2, nullptr, nullptr, 0) == hipSuccess && ge) {
    (void)hipGraphDestroy(g2);
    w.graph_exec = ge;
    HIPCHK(e, hipGraphLaunch(w.graph_exec, s));
    return use.release();
  }
  if (g2) (void)hipGraphDestroy(g2);
  w.graph_key.clear();                    // capture is an optimisation only: this descriptor runs eagerly
  if (r) return r;
  if (int r2 = run_device_pipeline(e, w, in, raw_total, key_total, out_dev, s, false, now)) return r2;
  return use.release();
}

int zke_verify_batch_async(zke_engine* e, const zke_batch* in, zke_result* out, uint64_t* ticket) {
  if (!e) return ZKE_E_ARG;
  HostBatch d;
  if (int r = host_batch(d, "zke_verify_batch_async", out, in)) return r;
  if (!ticket) return fail(e, ZKE_E_ARG, "zke_verify_batch_async: null ticket");
  return submit_host_batch(e, d, out, ticket);
}

int zke_batch_wait(zke_engine* e, uint64_t ticket) {
  if (!e) return ZKE_E_ARG;
  std::shared_lock<std::shared_mutex> sh(e->big);
  const uint32_t slot = (uint32_t)(ticket & 63);
  if (slot >= e->slots.size()) return fail(e, ZKE_E_ARG, "zke_batch_wait: no such ticket");
  Slot& w = *e->slots[slot];
  std::lock_guard<std::mutex> g(w.mu);
  if ((ticket >> 6) > w.host_gen) return fail(e, ZKE_E_ARG, "zke_batch_wait: no such ticket");
  if ((ticket >> 6) <= w.host_retired) return 0;        // delivered already (waited for before, or retired by the slot's next batch)
  HIPCHK(e, hipSetDevice(e->device));
  int cap_rc = 0;
  if (int r = retire_host(e, w, &cap_rc)) return r;
  return cap_rc;
}

int zke_verify_emails_with_regex_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_lists* lists,
                                       zke_result* out, uint64_t* ticket) {
  if (!e) return ZKE_E_ARG;
  if (!ticket) return fail(e, ZKE_E_ARG, "zke_verify_emails_async: null pointer");
  HostBatch d;
  if (int r = host_batch(d, "zke_verify_emails_async", out, emails, n, lists)) return r;
  return submit_host_batch(e, d, out, ticket);
}

int zke_verify_emails_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, zke_result* out, uint64_t* ticket) {
  return zke_verify_emails_with_regex_async(e, emails, n, nullptr, out, ticket);
}

int zke_verify_emails_with_regex(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_lists* lists, zke_result* out) {
  uint64_t ticket = 0;
  if (int r = zke_verify_emails_with_regex_async(e, emails, n, lists, out, &ticket)) return r;
  return n ? zke_batch_wait(e, ticket) : 0;
}

int zke_verify_emails(zke_engine* e, const zke_email_ref* emails, uint32_t n, zke_result* out) {
  return zke_verify_emails_with_regex(e, emails, n, nullptr, out);
}

int zke_verify_batch(zke_engine* e, const zke_batch* in, zke_result* out, zke_debug_out* dbg) {
  if (!e) return ZKE_E_ARG;
  HostBatch d;
  if (int r = host_batch(d, "zke_verify_batch", out, in)) return r;
  return submit_host_batch(e, d, out, nullptr, dbg);
}

// ---- single-e-mail wrappers: a batch of one through the gathering entry (config 1 and API-shape parity)
int zke_verify_email(zke_engine* e, const uint8_t* raw, size_t raw_len, const char* from_domain, size_t domain_len,
                     const uint8_t* key, size_t key_len, uint32_t key_type, uint32_t external_input_null, zke_result* out) {
  const zke_email_ref one{raw, raw_len, from_domain, domain_len, key, key_len, key_type, external_input_null};
  return zke_verify_emails_with_regex(e, &one, 1, nullptr, out);
}

int zke_verify_email_with_regex(zke_engine* e, const uint8_t* raw, size_t raw_len, const char* from_domain, size_t domain_len,
                                const uint8_t* key, size_t key_len, uint32_t key_type, uint32_t external_input_null,
                                const zke_regex_part* header_parts, uint32_t n_header_parts,
                                const zke_regex_part* body_parts, uint32_t n_body_parts, zke_result* out) {
  if (!e) return ZKE_E_ARG;
  if ((n_header_parts && !header_parts) || (n_body_parts && !body_parts)) return fail(e, ZKE_E_ARG, "zke_verify_email_with_regex: null pointer");
  std::vector<uint32_t> hids, bids, cap_off{0}, str_off{0};
  std::vector<uint8_t> blob;
  // every pair this call registers or finds stays pinned until the batch has run: with the registry at its cap another
  // thread's registration evicts the least recently used transient pair and the id is handed out again
  struct Pins { zke_engine* e; std::vector<uint32_t> ids; ~Pins() { if (!ids.empty()) dfa_unpin(e, ids); } } pinned{e, {}};
  for (int side = 0; side < 2; side++) {
    const zke_regex_part* parts = side ? body_parts : header_parts;
    const uint32_t np = side ? n_body_parts : n_header_parts;
    for (uint32_t k = 0; k < np; k++) {
      const zke_regex_part& p = parts[k];
      if ((p.fwd_len && !p.fwd) || (p.bwd_len && !p.bwd) || (p.n_captures && (!p.captures || !p.capture_lens)))
        return fail(e, ZKE_E_ARG, "zke_verify_email_with_regex: null pointer in a part");
      uint32_t id = 0;
      // the same pair gets the same id: a hash lookup, not a parse; pairs registered here are the evictable ones
      if (int r = dfa_register_impl(e, p.fwd, p.fwd_len, p.bwd, p.bwd_len, &id, true)) return r;
      pinned.ids.push_back(id);
      (side ? bids : hids).push_back(id);
      for (uint32_t c = 0; c < p.n_captures; c++) {
        if (p.capture_lens[c] && !p.captures[c]) return fail(e, ZKE_E_ARG, "zke_verify_email_with_regex: null capture");
        blob.insert(blob.end(), p.captures[c], p.captures[c] + p.capture_lens[c]);
        str_off.push_back((uint32_t)blob.size());
      }
      cap_off.push_back((uint32_t)str_off.size() - 1);
    }
  }
  if (blob.empty()) blob.push_back(0);          // (captures that are all empty strings still want a blob pointer)
  const zke_email_ref one{raw, raw_len, from_domain, domain_len, key, key_len, key_type, external_input_null};
  const zke_regex_lists lists{n_header_parts, hids.data(), n_body_parts, bids.data(), cap_off.data(), str_off.data(), blob.data()};
  return zke_verify_emails_with_regex(e, &one, 1, &lists, out);
}

// ---- signature scan and key selection (include/zkemail_amd.h; kernel: sigscan.hip.h)
int zke_scan_signatures_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, uint32_t max_sigs, zke_sig_scan* out, uint64_t* ticket) {
  static const char who[] = "zke_scan_signatures";
  if (!e) return ZKE_E_ARG;
  if (!out || !ticket || (n && !emails)) return arg_error(who, "null pointer");
  if (max_sigs < 1 || max_sigs > ZKE_SCAN_MAX_SIGS) return arg_error(who, "max_sigs must be 1 .. ZKE_SCAN_MAX_SIGS");
  if ((uint64_t)n * max_sigs >= (1ull << 21)) return arg_error(who, "n * max_sigs must stay below 2^21 (32-bit selector offsets): split the batch");
  out->scan_status_need = (size_t)n * 4; out->sig_off_need = (size_t)n + 1; out->sigs_need = 0; out->sel_blob_need = 0; out->n_sigs = 0;
  if (out->scan_status_cap < out->scan_status_need || out->sig_off_cap < out->sig_off_need) {
    g_err = std::string(who) + ": a zke_sig_scan buffer is smaller than its *_need";
    return ZKE_E_NOMEM;
  }
  if ((n && !out->scan_status) || !out->sig_off || (out->sigs_cap && !out->sigs) || (out->sel_blob_cap && !out->sel_blob))
    return arg_error(who, "null buffer in zke_sig_scan");
  out->sig_off[0] = 0;
  std::vector<zke_email_ref> refs(emails, emails + n);              // the key fields are ignored: the image has no key section
  for (zke_email_ref& m : refs) { m.key = nullptr; m.key_len = 0; m.key_type = ZKE_KEY_RSA; m.external_input_null = 0; }
  HostBatch d;
  if (int r = host_batch(d, who, reinterpret_cast<const zke_result*>(out), refs.data(), n, nullptr)) return r;
  const ScanReq q{max_sigs, out};
  d.scan = &q;
  return submit_host_batch(e, d, nullptr, ticket);
}

int zke_scan_signatures(zke_engine* e, const zke_email_ref* emails, uint32_t n, uint32_t max_sigs, zke_sig_scan* out) {
  uint64_t ticket = 0;
  if (int r = zke_scan_signatures_async(e, emails, n, max_sigs, out, &ticket)) return r;
  return n ? zke_batch_wait(e, ticket) : 0;
}

int zke_select_keys_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off, const zke_key_ref* keys,
                          zke_result* out, uint32_t* chosen, uint64_t* ticket) {
  static const char who[] = "zke_select_keys";
  if (!e) return ZKE_E_ARG;
  if (!ticket || (n && (!emails || !cand_off || !out || !chosen))) return arg_error(who, "null pointer");
  if (n && !rising(cand_off, n)) return arg_error(who, "cand_off is not non-decreasing");
  const uint32_t base = n ? cand_off[0] : 0, M = n ? cand_off[n] - base : 0;
  if (M >> 31) return arg_error(who, "2^31 candidates or more");
  if (M && !keys) return arg_error(who, "null pointer");
  // ONE batch of the (e-mail, candidate key) pairs: the raw e-mail and the domain by reference, once per candidate
  std::vector<zke_email_ref> refs(M);
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t k = cand_off[i]; k < cand_off[i + 1]; k++) {
      zke_email_ref& m = refs[k - base];
      m = emails[i];
      m.key = keys[k].key; m.key_len = keys[k].key_len; m.key_type = keys[k].key_type;
    }
  HostBatch d;
  if (int r = host_batch(d, who, out, refs.data(), M, nullptr)) return r;
  if (!M) {            // no candidate anywhere: nothing to run
    const std::vector<uint32_t> off((size_t)n + 1, 0u);
    if (n) fold_selection(nullptr, off, out, chosen);
    return submit_host_batch(e, d, out, ticket);
  }
  const SelectReq q{cand_off, n, out, chosen};
  d.sel = &q;
  return submit_host_batch(e, d, out, ticket);
}

int zke_select_keys(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off, const zke_key_ref* keys,
                    zke_result* out, uint32_t* chosen) {
  uint64_t ticket = 0;
  if (int r = zke_select_keys_async(e, emails, n, cand_off, keys, out, chosen, &ticket)) return r;
  return n ? zke_batch_wait(e, ticket) : 0;
}

// ---- key records (include/zkemail_amd.h; kernels: keyrec.hip.h)
namespace {
// The checks both entries share, before anything is staged; fills the needs.  A record longer than ZKE_KEYREC_MAX_BYTES is not
// read: one byte more than the limit is staged, which is all the kernel needs to say so.
int keyrec_args(const char* who, const zke_keyrec_ref* recs, uint32_t m, uint32_t mode, zke_keyrec_out* out) {
  if (!out || (m && !recs)) return arg_error(who, "null pointer");
  if (mode != ZKE_KEYREC_ARCHIVE && mode != ZKE_KEYREC_DNS) return arg_error(who, "mode must be ZKE_KEYREC_ARCHIVE or ZKE_KEYREC_DNS");
  if (m >= (1u << 19)) return arg_error(who, "2^19 records or more (32-bit key offsets): split the batch");
  for (uint32_t i = 0; i < m; i++)
    if (recs[i].len && !recs[i].txt) return arg_error(who, "null buffer with a length");
  out->infos_need = m; out->keys_need = 0;
  if (out->infos_cap < m) { g_err = std::string(who) + ": zke_keyrec_out.infos is smaller than infos_need"; return ZKE_E_NOMEM; }
  if ((m && !out->infos) || (out->keys_cap && !out->keys)) return arg_error(who, "null buffer in zke_keyrec_out");
  return 0;
}
inline size_t keyrec_staged(size_t len) { return std::min<size_t>(len, (size_t)ZKE_KEYREC_MAX_BYTES + 1); }
}  // namespace

int zke_decode_key_records_async(zke_engine* e, const zke_keyrec_ref* recs, uint32_t m, uint32_t mode, zke_keyrec_out* out, uint64_t* ticket) {
  static const char who[] = "zke_decode_key_records";
  if (!e) return ZKE_E_ARG;
  if (!ticket) return arg_error(who, "null pointer");
  if (int r = keyrec_args(who, recs, m, mode, out)) return r;
  std::vector<zke_email_ref> refs(m);                 // the records travel as the image's raw section: no domains, no keys
  for (uint32_t i = 0; i < m; i++) { refs[i] = zke_email_ref{}; refs[i].raw = recs[i].txt; refs[i].raw_len = keyrec_staged(recs[i].len); }
  HostBatch d;
  if (int r = host_batch(d, who, reinterpret_cast<const zke_result*>(out), refs.data(), m, nullptr)) return r;
  const KeyrecReq q{mode, out};
  d.keyrec = &q;
  return submit_host_batch(e, d, nullptr, ticket);
}

int zke_decode_key_records(zke_engine* e, const zke_keyrec_ref* recs, uint32_t m, uint32_t mode, zke_keyrec_out* out) {
  uint64_t ticket = 0;
  if (int r = zke_decode_key_records_async(e, recs, m, mode, out, &ticket)) return r;
  return m ? zke_batch_wait(e, ticket) : 0;
}

int zke_select_keys_from_records_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off,
                                       const zke_keyrec_ref* recs, uint32_t mode, zke_result* out, uint32_t* chosen,
                                       zke_keyrec_out* keys_out, uint64_t* ticket) {
  static const char who[] = "zke_select_keys_from_records";
  if (!e) return ZKE_E_ARG;
  if (!ticket || !keys_out || (n && (!emails || !cand_off || !out || !chosen))) return arg_error(who, "null pointer");
  if (n && !rising(cand_off, n)) return arg_error(who, "cand_off is not non-decreasing");
  const uint32_t base = n ? cand_off[0] : 0, M = n ? cand_off[n] - base : 0;
  if (int r = keyrec_args(who, recs ? recs + base : nullptr, M, mode, keys_out)) return r;
  // ONE batch of the (e-mail, candidate) pairs, as zke_select_keys; the key section of its image holds the candidates' records
  std::vector<zke_email_ref> refs(M);
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t k = cand_off[i]; k < cand_off[i + 1]; k++) {
      zke_email_ref& m = refs[k - base];
      m = emails[i];
      m.key = recs[k].txt; m.key_len = keyrec_staged(recs[k].len); m.key_type = ZKE_KEY_RSA;
    }
  HostBatch d;
  if (int r = host_batch(d, who, out, refs.data(), M, nullptr)) return r;
  if (!M) {            // no candidate anywhere: nothing to run
    const std::vector<uint32_t> off((size_t)n + 1, 0u);
    if (n) fold_selection(nullptr, off, out, chosen);
    return submit_host_batch(e, d, out, ticket);
  }
  const SelectReq q{cand_off, n, out, chosen};
  const KeyrecReq kq{mode, keys_out};
  d.sel = &q; d.keyrec = &kq;
  return submit_host_batch(e, d, out, ticket);
}

int zke_select_keys_from_records(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off,
                                 const zke_keyrec_ref* recs, uint32_t mode, zke_result* out, uint32_t* chosen, zke_keyrec_out* keys_out) {
  uint64_t ticket = 0;
  if (int r = zke_select_keys_from_records_async(e, emails, n, cand_off, recs, mode, out, chosen, keys_out, &ticket)) return r;
  return n ? zke_batch_wait(e, ticket) : 0;
}

// ---- capture extraction (include/zkemail_amd.h; kernels: capture.hip.h)
int zke_capture_validate(const uint8_t* prog, size_t len, uint32_t* detail) {
  if (!detail || (len && !prog)) return ZKE_E_ARG;
  HostCapture h;
  *detail = parse_capture_program(prog, len, h);
  return 0;
}

int zke_capture_register(zke_engine* e, const uint8_t* prog, size_t len, uint32_t* out_id) {
  if (!e || !out_id || (len && !prog)) return ZKE_E_ARG;
  const uint64_t hsh = pair_hash(prog, len, nullptr, 0);
  auto lookup = [&]() {
    auto range = e->capture_index.equal_range(hsh);
    for (auto it = range.first; it != range.second; ++it) {
      const RegisteredCapture* c = e->captures[it->second];
      if (c && c->copy.size() == len && (!len || !memcmp(c->copy.data(), prog, len))) { *out_id = it->second; return true; }
    }
    return false;
  };
  {
    std::shared_lock<std::shared_mutex> rl(e->reg_mu);
    if (lookup()) return 0;
  }
  HIPCHK(e, hipSetDevice(e->device));
  RegisteredCapture* rc = new RegisteredCapture();
  auto discard = [&]() { rc->blob.release(); delete rc; };
  rc->copy.assign(prog, prog + len);
  rc->hash = hsh;
  HostCapture h;
  rc->detail = parse_capture_program(prog, len, h);
  if (!rc->detail) {
    const size_t tb = (h.table.size() * 4 + 7) & ~(size_t)7, eb = h.eps.size() * 8;
    if (int r = rc->blob.ensure(tb + eb)) { discard(); return fail(e, r, "hipMalloc"); }
    hipError_t he = hipMemcpy(rc->blob.p, h.table.data(), h.table.size() * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(rc->blob.as<uint8_t>() + tb, h.eps.data(), eb, hipMemcpyHostToDevice);
    if (he != hipSuccess) { discard(); return fail(e, ZKE_E_DEVICE, "capture program upload", he); }
    rc->dev.n_states = h.n_states; rc->dev.n_groups = h.n_groups; rc->dev.start = h.start; rc->dev.words64 = (uint32_t)h.eps.size();
    rc->dev.off = rc->blob.as<uint32_t>();
    rc->dev.st = rc->blob.as<uint32_t>() + h.n_states + 1;
    rc->dev.eps = reinterpret_cast<const uint64_t*>(rc->blob.as<uint8_t>() + tb);
  }
  std::unique_lock<std::shared_mutex> rl(e->reg_mu);
  if (lookup()) { discard(); return 0; }             // another thread was first
  uint32_t live = 0;
  for (const auto* c : e->captures) live += c != nullptr;
  if (live >= e->opt.max_dfas) { discard(); return fail(e, ZKE_E_NOMEM, "capture registry full (zke_options.max_dfas): zke_capture_unregister programs no longer needed"); }
  uint32_t id = 0;
  while (id < e->captures.size() && e->captures[id]) id++;
  if (id == e->captures.size()) e->captures.push_back(nullptr);
  e->captures[id] = rc;
  e->capture_index.emplace(hsh, id);
  *out_id = id;
  return 0;
}

int zke_capture_status(zke_engine* e, uint32_t id, uint32_t* detail) {
  if (!e || !detail) return ZKE_E_ARG;
  std::shared_lock<std::shared_mutex> rl(e->reg_mu);
  if (id >= e->captures.size() || !e->captures[id]) return fail(e, ZKE_E_DFA, "zke_capture_status: id is not registered");
  *detail = e->captures[id]->detail;
  return 0;
}

int zke_capture_unregister(zke_engine* e, uint32_t id) {
  if (!e) return ZKE_E_ARG;
  std::unique_lock<std::shared_mutex> ex(e->big);         // no submission in progress, nothing in flight that could read the tables
  HIPCHK(e, hipSetDevice(e->device));
  if (int r = drain_engine(e, false)) return r;
  std::unique_lock<std::shared_mutex> rl(e->reg_mu);
  if (id >= e->captures.size() || !e->captures[id]) return fail(e, ZKE_E_DFA, "zke_capture_unregister: id is not registered");
  RegisteredCapture* c = e->captures[id];
  auto range = e->capture_index.equal_range(c->hash);
  for (auto it = range.first; it != range.second; ++it)
    if (it->second == id) { e->capture_index.erase(it); break; }
  c->blob.release();
  delete c;
  e->captures[id] = nullptr;
  return 0;
}

namespace {
// the sizes an extraction over n e-mails needs, written back; ZKE_E_NOMEM when a buffer of known size is too small
int check_capture_out(zke_capture_out* o, uint32_t n, uint32_t P, uint32_t G, const char* who) {
  if (!o) return arg_error(who, "null zke_capture_out");
  const size_t NP = (size_t)n * P, NG = (size_t)n * G;
  o->spans_need = NG * 2; o->flags_need = NG; o->cap_off_need = NP + 1; o->cap_str_off_need = NG + 1;
  o->cap_blob_need = 0; o->n_strings = 0;
  // string offsets are 32-bit, as the verify entry's tables are: what n * G spans of ZKE_CAP_MAX_SPAN bytes could not address is refused
  if ((uint64_t)NG * ZKE_CAP_MAX_SPAN > 0xFFFFFFFFull) return arg_error(who, "n x groups beyond what 32-bit string offsets address (n * G * ZKE_CAP_MAX_SPAN must stay below 4 GiB): split the batch");
  if (o->spans_cap < o->spans_need || o->flags_cap < o->flags_need || o->cap_off_cap < o->cap_off_need || o->cap_str_off_cap < o->cap_str_off_need) {
    g_err = std::string(who) + ": a zke_capture_out buffer is smaller than its *_need";
    return ZKE_E_NOMEM;
  }
  if (!o->spans || !o->flags || !o->cap_off || !o->cap_str_off || (o->cap_blob_cap && !o->cap_blob)) return arg_error(who, "null buffer in zke_capture_out");
  return 0;
}
}  // namespace

int zke_extract_captures_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                               uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                               zke_capture_out* caps, uint64_t* ticket) {
  static const char who[] = "zke_extract_captures";
  if (!e) return ZKE_E_ARG;
  if (!ticket || !caps || (n_header_parts && !header_parts) || (n_body_parts && !body_parts)) return arg_error(who, "null pointer");
  const uint32_t P = n_header_parts + n_body_parts;
  if (P == 0 || P > ZKE_CAP_MAX_PARTS || n_header_parts > ZKE_CAP_MAX_PARTS) return arg_error(who, "1 .. ZKE_CAP_MAX_PARTS parts");
  CaptureReq q;
  q.P = P; q.n_header_parts = n_header_parts; q.out = caps;
  q.dfa_ids.resize(P);
  for (uint32_t p = 0; p < P; p++) {
    const zke_capture_part& cp = p < n_header_parts ? header_parts[p] : body_parts[p - n_header_parts];
    q.dfa_ids[p] = cp.dfa_id;
    if (int r = capture_part_shape(q, p, cp.prog_id, cp.groups, cp.n_groups, who)) return r;
  }
  if (int r = check_capture_out(caps, n, P, q.G, who)) return r;
  zke_regex_lists lists{n_header_parts, q.dfa_ids.data(), n_body_parts, q.dfa_ids.data() + n_header_parts, nullptr, nullptr, nullptr};
  HostBatch d;
  if (int r = host_batch(d, who, out, emails, n, &lists)) return r;
  d.cap = &q;
  return submit_host_batch(e, d, out, ticket);
}

int zke_extract_captures(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                         uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                         zke_capture_out* caps) {
  uint64_t ticket = 0;
  if (int r = zke_extract_captures_async(e, emails, n, header_parts, n_header_parts, body_parts, n_body_parts, out, caps, &ticket)) return r;
  return n ? zke_batch_wait(e, ticket) : 0;
}

int zke_capture_batch(zke_engine* e, uint32_t dfa_id, uint32_t prog_id, const uint32_t* groups, uint32_t n_groups,
                      const uint8_t* hay_blob, const uint64_t* hay_off, uint32_t n, uint32_t* matches, zke_capture_out* caps) {
  static const char who[] = "zke_capture_batch";
  if (!e) return ZKE_E_ARG;
  if (!caps || (n && (!hay_off || !matches)) || (n && hay_off[n] > hay_off[0] && !hay_blob)) return arg_error(who, "null pointer");
  if (n && (!rising(hay_off, n) || hay_off[n] - hay_off[0] > (1ull << 32))) return arg_error(who, "offset array is not non-decreasing, or the haystacks exceed 4 GiB");
  for (uint32_t i = 0; i < n; i++) if (hay_off[i + 1] - hay_off[i] >= (1ull << 31)) return arg_error(who, "haystack of 2 GiB or more");
  CaptureReq q;
  q.P = 1; q.n_header_parts = 1; q.out = caps;
  if (int r = capture_part_shape(q, 0, prog_id, groups, n_groups, who)) return r;
  if (int r = check_capture_out(caps, n, 1, q.G, who)) return r;
  if (n == 0) return 0;
  std::shared_lock<std::shared_mutex> sh(e->big);      // from the registry lookups to the last launch: no table is freed meanwhile
  std::lock_guard<std::mutex> g(e->misc_mu);
  HIPCHK(e, hipSetDevice(e->device));
  capture_resolve(e, q);
  PartInfo pi{};
  {
    std::shared_lock<std::shared_mutex> rl(e->reg_mu);
    const RegisteredDfa* rd = dfa_id < e->dfas.size() ? e->dfas[dfa_id] : nullptr;
    if (rd) { pi.detail = rd->detail; pi.dev = rd->valid ? rd->dev.as<RegexDev>() : nullptr; }
  }
  // the building blocks run in buffers of their own on slot 0's stream
  const uint64_t base0 = hay_off[0], total = hay_off[n] - base0;
  CapBufs tmp;
  DevBuf dhay, doff, dparts;
  std::vector<uint8_t> fixed;
  int r = 0;
  hipError_t he = hipSuccess;
  tmp.L = cap_layout(n, 1, q.G, caps->cap_blob_cap);
  const CapLayout& L = tmp.L;
  hipStream_t s = e->stream;
  auto done = [&](int rc) { dhay.release(); doff.release(); dparts.release(); tmp.release(); return rc; };
  if ((r = dhay.ensure((size_t)total + 64)) || (r = doff.ensure((size_t)(n + 1) * 8)) || (r = dparts.ensure((size_t)n * sizeof(PartRes))) ||
      (r = ensure_capture_buffers(e, tmp, n, 1, q.G, caps->cap_blob_cap, q.needs_work)))
    return done(fail(e, r, "zke_capture_batch: allocation"));
  std::vector<uint64_t> rel(n + 1);
  for (uint32_t i = 0; i <= n; i++) rel[i] = hay_off[i] - base0;
  if (total) he = hipMemcpyAsync(dhay.p, hay_blob + base0, (size_t)total, hipMemcpyHostToDevice, s);
  if (he == hipSuccess) he = hipMemsetAsync(dhay.as<uint8_t>() + total, 0, 64, s);         // the DFA walk loads 16 bytes at a time
  if (he == hipSuccess) he = hipMemcpyAsync(doff.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s);
  if (he != hipSuccess) { (void)hipStreamSynchronize(s); return done(fail(e, ZKE_E_DEVICE, "zke_capture_batch: copy", he)); }
  CapFindArgs fa{};
  fa.d.re = pi.dev; fa.d.P = 1; fa.d.out = dparts.as<PartRes>(); fa.d.idle = 0xFFFFFFFFu; fa.d.decode_detail = pi.detail;
  fa.hay_blob = dhay.as<uint8_t>(); fa.hay_off = doff.as<uint64_t>(); fa.n = n;
  hipLaunchKernelGGL(capture_find_kernel, dim3((n + 255) / 256), dim3(256), 1024, s, fa);
  r = launch_capture(e, tmp, q, n, true, DfaArgs{}, fa.hay_blob, fa.hay_off, dparts.as<PartRes>(), nullptr, s);
  std::vector<PartRes> prs(n);
  if (!r) {
    he = hipMemcpyAsync(tmp.h_cap.p, tmp.cap.p, L.fixed_end, hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipMemcpyAsync(prs.data(), dparts.p, (size_t)n * sizeof(PartRes), hipMemcpyDeviceToHost, s);
  }
  const hipError_t hs = hipStreamSynchronize(s);
  if (r) return done(r);
  if (he != hipSuccess || hs != hipSuccess) return done(fail(e, ZKE_E_DEVICE, "zke_capture_batch", he != hipSuccess ? he : hs));
  const uint32_t* codes = reinterpret_cast<const uint32_t*>(tmp.h_cap.as<uint8_t>() + L.codes);
  for (uint32_t i = 0; i < n; i++) {
    const PartRes& pr = prs[i];
    const bool undecodable = pr.code == PART_DECODE_FAIL;
    matches[4 * i] = undecodable ? pr.count : (pr.code ? pr.code : codes[i]);
    matches[4 * i + 1] = undecodable ? 0 : pr.count; matches[4 * i + 2] = pr.start; matches[4 * i + 3] = pr.end;
  }
  return done(deliver_captures(e, tmp, caps, s));
}

}  // extern "C"
