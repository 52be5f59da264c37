// host_entry.hip.h — the entries whose batch lies in host memory: the batch descriptor and its checks, the packed image into a
// slot (host_stage.hip.h), upload, launches (pipeline.hip.h), and the slot's debt of a delivery into the caller's buffers
// (host_deliver.hip.h).  Stands for the reference's callers, `&[Email]` into verify_email / verify_email_with_regex
// (core/src/circuits.rs:9-68), and for what comes before a key is known: scan, key records, selection, captures.  Included by engine.hip
// behind pipeline.hip.h, registry.hip.h and host_deliver.hip.h (one translation unit); the synchronous building blocks: host_blocks.hip.h.
#pragma once

#ifndef ZKE_HOST_COPY_STREAM
#define ZKE_HOST_COPY_STREAM 1     // 0: every input image is copied on its slot's own stream
#endif

namespace {

inline uint64_t host_scratch_off(const uint64_t* raw_off, uint32_t i) { return scratch_offset(raw_off[i] - raw_off[0], i); }

// Host-entry buffers of one slot: the packed input image (pinned and in HBM) and the records (HBM and pinned).
int ensure_host_buffers(zke_engine* e, Slot& w, size_t image_bytes, uint32_t n) {
  int r = 0;
  if ((r = w.h_image.ensure(image_bytes)) || (r = w.d_image.ensure(image_bytes)) ||
      (r = w.h_results.ensure((size_t)n * sizeof(zke_result))) || (r = w.d_results.ensure((size_t)n * sizeof(zke_result))))
    return fail(e, r, "host-entry staging allocation");
  return 0;
}

// ---- signature scan and key selection (sigscan.hip.h; include/zkemail_amd.h)
struct ScanReq { uint32_t max_sigs; zke_sig_scan* out; };
struct SelectReq { const uint32_t* cand_off; uint32_t n; zke_result* out; uint32_t* chosen; };
// ---- key records (keyrec.hip.h).  Alone: the batch's "raw e-mails" are the records, keyrec_kernel runs instead of the verify
// pipeline.  With a SelectReq: the image's key section holds the records, and the decode + pack launches in front of the front end
// replace it by the decoded keys (zke_select_keys_from_records).
struct KeyrecReq { uint32_t mode; zke_keyrec_out* out; };
// ---- body extraction (bodyext.hip.h): the batch's raw section holds the e-mails, body_extract_kernel runs instead of the verify pipeline
struct BodyReq { uint32_t flags; zke_body_out* out; };

// ---- mixed regex batches (zke_verify_emails_mixed; plan: mixed_plan.hip.h, kernels: regex_mixed.hip.h).  The entry checks the
// arguments and measures (`shape`, `counts`); mixed_resolve builds the plan once the registry can be read; submit_host stages it.
struct MixedReq {
  const zke_regex_mixed* in = nullptr;
  uint32_t n = 0;
  std::vector<MixedConfigIn> counts;    // [n_configs]
  MixedShape shape;
  MixedPlan plan;
};
// The configs' parts resolved against the registry and the plan built from them.  The caller holds `big` (shared) from here until the
// batch is enqueued, as for capture_resolve: the tables the segments point to cannot be freed before the launches that read them.
int mixed_resolve(zke_engine* e, MixedReq& q) {
  std::vector<MixedPartIn> parts;
  parts.reserve(q.shape.n_segs);
  {
    std::shared_lock<std::shared_mutex> rl(e->reg_mu);
    for (uint32_t c = 0; c < q.in->n_configs; c++) {
      const zke_regex_config& cf = q.in->configs[c];
      for (uint32_t p = 0; p < cf.n_header_parts + cf.n_body_parts; p++) {
        const PartInfo pi = part_info(e, p >= cf.n_header_parts ? cf.body_part_ids[p - cf.n_header_parts] : cf.header_part_ids[p]);
        parts.push_back(MixedPartIn{(uint64_t)(uintptr_t)pi.dev, pi.lds_bytes, pi.idle, pi.detail});
      }
    }
  }
  if (const char* why = mixed_plan_build(q.in->config_of, q.n, q.counts.data(), q.in->n_configs, parts.data(), e->opt.dfa_mapping, q.plan))
    return fail(e, ZKE_E_ARG, why);
  return 0;
}

// ---- mixed extractions (zke_extract_captures_mixed; plan: mixed_plan.hip.h, kernels: capture_mixed.hip.h).  The regex stage in front
// of the capture launches is a mixed batch's (`verify`, over the parts' DFA ids, no capture tables); on top of it the ragged columns
// (`plan`) and the config-major part table, whose programs capmix_resolve copies out of the registry.
struct CapMixedReq {
  MixedReq verify;
  zke_regex_mixed lists{};               // what `verify` plans over: the configs' DFA ids, the caller's config_of
  std::vector<zke_regex_config> id_lists;
  std::vector<uint32_t> dfa_ids, prog_ids, n_groups;      // config-major, header parts first
  std::vector<CapPartDev> part;          // the device part table (groups and gbase: the entry; code and prog: capmix_resolve)
  CapMixedPlan plan;
  bool needs_work = false;               // some program's rows do not fit LDS
  zke_capture_out* out = nullptr;
  zke_capture_origin* org = nullptr;
  bool origin_launch() const { return org && plan.shape.body_groups; }
  CapMixedImage image(uint32_t n) const { return capmix_image(n, lists.n_configs, plan.shape, sizeof(CapPartDev)); }
};
// Under `big` (shared), like capture_resolve: the pointers copied here stay valid until the batch is enqueued.
void capmix_resolve(zke_engine* e, CapMixedReq& q) {
  std::shared_lock<std::shared_mutex> rl(e->reg_mu);
  q.needs_work = false;
  for (size_t k = 0; k < q.part.size(); k++)
    if (capture_resolve_part(e, q.part[k], q.prog_ids[k])) q.needs_work = true;
}

// ---- output encoding (zke_verify_emails_encoded; plan: encode_plan.hip.h, kernel: encode.hip.h): the plan — the jobs, the places, the
// exact size of the blob — is built by the entry before anything is staged; the jobs and the external-input table ride in the batch's
// input image (EncImage, behind a mixed batch's plan), the matches are the capture tables the regex stage reads.
struct EncodeReq {
  zke_encoded_out* out = nullptr;
  EncodePlan plan;
  const uint32_t* ext_str_off = nullptr;
  const uint8_t* ext_blob = nullptr;
  // zke_extract_captures_encoded: the plan is the device's (capture_lossy.hip.h).  `plan` then holds no jobs, only what the external
  // inputs measure; ext_off[n + 1] rides in the image where the jobs would (a job is larger than a word: n jobs hold n + 1 words);
  // bytes_cap: the capacity of the encodings on the device.
  bool device_plan = false;
  uint32_t n = 0;
  const uint32_t* ext_off = nullptr;
  uint64_t bytes_cap = 0;
  EncImage image() const { return enc_image(device_plan ? n : (uint32_t)plan.jobs.size(), plan.ext_strs, plan.ext_bytes); }
};

// Deliver a host batch that was enqueued in this slot and not waited for yet: wait for its last D2H, pay what is owed for it.
// Caller holds the slot's lock.
int retire_host(zke_engine* e, Slot& w, int* cap_rc = nullptr) {
  if (w.host_retired == w.host_gen) return 0;
  w.host_retired = w.host_gen;                       // whatever happens below, the batch is no longer pending
  const PendingDelivery d = std::move(w.owed);
  w.owed = PendingDelivery{};
  HIPCHK(e, hipEventSynchronize(w.host_done));
  return deliver_pending(e, w, d, cap_rc);
}

int arg_error(const char* who, const char* what) { g_err = std::string(who) + ": " + what; return ZKE_E_ARG; }
int nomem_error(const char* who, const char* what) { g_err = std::string(who) + ": " + what; return ZKE_E_NOMEM; }      // a buffer of known size is too small
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

// A host batch, checked and measured for the staging image by host_batch(): packed (zke_batch) or gathered (zke_email_ref[n]).  The requests say
// what is asked; the three that are not const are completed against the registry by submit_host_batch, under `big`; submit_host writes through none.
struct HostBatch {
  zke_batch b{};                        // n, the regex section, (packed) the caller's blobs and offsets; capture tables only if any
  const zke_email_ref* refs = nullptr;  // the gathered shape's e-mails (nullptr: packed)
  CaptureReq* cap = nullptr;            // zke_extract_captures: the extraction that rides on this (regex) batch
  const ScanReq* scan = nullptr;        // zke_scan_signatures: sigscan_kernel runs instead of the verify pipeline
  const SelectReq* sel = nullptr;       // zke_select_keys: the batch's entries are (e-mail, candidate key) pairs, folded on delivery
  const KeyrecReq* keyrec = nullptr;    // key records: decoded instead of the verify pipeline, or (with sel) in front of it
  const BodyReq* body = nullptr;        // zke_extract_bodies: body_extract_kernel runs instead of the verify pipeline
  MixedReq* mixed = nullptr;            // zke_verify_emails_mixed: a regex batch whose part lists are the configs' (b's own are empty)
  CapMixedReq* capmix = nullptr;        // zke_extract_captures_mixed: the extraction that rides on this mixed batch (mixed == &capmix->verify)
  const EncodeReq* enc = nullptr;       // zke_verify_emails_encoded: the encode and digest launches behind this batch's records
  uint64_t raw_total = 0, dom_total = 0, key_total = 0, raw_base = 0, dom_base = 0, key_base = 0;   // blob bytes; off[0] of packed offsets
  size_t cap_words = 0, cap_strs = 0, cap_bytes = 0;      // entries of cap_off and cap_str_off, bytes of cap_blob (0: no tables)
  PlanSections S{};                     // the plan sections behind L.mixed and the image: layout_host_batch, once
  ImageLayout L{};
};
// The image of a batch that has been measured and whose plan sections are all known: the sections (host_stage.hip.h), then the image
// around them.  Once per batch: host_batch() ends with it, unless the entry has an encoding to add first and calls it itself (`lay_out`).
void layout_host_batch(HostBatch& d) {
  d.S = plan_sections(d.mixed ? mixed_image(d.b.n, d.mixed->shape) : MixedImage{}, d.capmix ? d.capmix->image(d.b.n) : CapMixedImage{},
                      d.enc ? d.enc->image() : EncImage{});
  d.L = image_layout(d.b.n, d.raw_total, d.dom_total, d.key_total, d.cap_words, d.cap_strs, d.cap_bytes, d.S.total);
}
// Both shapes.  Capture tables: a cap_off whose last entry is 0 holds no string and is no table (cap_str_off, cap_blob unread).
int measure_host_batch(HostBatch& d, const char* who, bool lay_out = true) {
  zke_batch& b = d.b;
  if (d.raw_total > (1ull << 40)) return arg_error(who, "raw e-mails beyond 1 TiB");
  const size_t NP = d.mixed ? (size_t)d.mixed->shape.J : b.with_regex ? (size_t)b.n * (b.n_header_parts + b.n_body_parts) : 0;
  if (NP && b.cap_off) {
    if (!rising(b.cap_off, NP)) return arg_error(who, "capture offset array is not non-decreasing");
    if (const uint32_t strs = b.cap_off[NP]) {
      if (!b.cap_str_off || !b.cap_blob) return arg_error(who, "capture strings without cap_str_off or cap_blob");
      if (!rising(b.cap_str_off, strs)) return arg_error(who, "capture offset array is not non-decreasing");
      d.cap_words = NP + 1; d.cap_strs = (size_t)strs + 1; d.cap_bytes = b.cap_str_off[strs];
    }
  }
  if (!d.cap_words) b.cap_off = nullptr, b.cap_str_off = nullptr, b.cap_blob = nullptr;
  if (lay_out) layout_host_batch(d);
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
// The gathered shape: the e-mails one by one, lists == nullptr for verify_email; `mixed` (checked and measured by its entry) instead
// of lists: the capture tables are its; `capmix`: its mixed extraction.  lay_out = false: the entry sets d.enc, then lays the image out itself.
int host_batch(HostBatch& d, const char* who, const zke_result* out, const zke_email_ref* refs, uint32_t n, const zke_regex_lists* lists,
               MixedReq* mixed = nullptr, CapMixedReq* capmix = nullptr, bool lay_out = true) {
  if (n && (!refs || !out)) return arg_error(who, "null pointer");
  d = HostBatch{zke_batch{n}, refs};
  d.capmix = capmix;
  if (mixed) {
    d.mixed = mixed;
    d.b.with_regex = 1;
    d.b.cap_off = mixed->in->cap_off; d.b.cap_str_off = mixed->in->cap_str_off; d.b.cap_blob = mixed->in->cap_blob;
  }
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
  return measure_host_batch(d, who, lay_out);
}

// What the slot will owe for the batch d: only a batch that is nothing but a verify hands the records over as they are.
PendingDelivery pending_delivery(const HostBatch& d, zke_result* out) {
  PendingDelivery p;
  if (!(d.scan || d.sel || d.keyrec || d.body)) { p.records = out; p.n = d.b.n; }
  if (d.sel) {
    p.sel_off.resize((size_t)d.sel->n + 1);
    for (uint32_t i = 0; i <= d.sel->n; i++) p.sel_off[i] = d.sel->cand_off[i] - d.sel->cand_off[0];
    p.sel_out = d.sel->out; p.sel_chosen = d.sel->chosen;
  }
  if (d.scan) p.scan = d.scan->out;
  if (d.keyrec) p.keyrec = d.keyrec->out;
  if (d.body) p.body = d.body->out;
  if (d.cap) { p.caps = d.cap->out; p.org = d.cap->org; }
  if (d.capmix) { p.caps = d.capmix->out; p.org = d.capmix->org; }
  if (d.enc) { p.enc = d.enc->out; p.enc_planned = d.enc->device_plan; }
  return p;
}

// ---- One host batch into a slot, stage by stage (submit_host below is the list); every stage reads the descriptor and writes the slot.
// 1. The buffers of every output the batch asks for (grow only; the layouts of the batch at hand).
int ensure_output_buffers(zke_engine* e, Slot& w, const HostBatch& d) {
  const uint32_t n = d.b.n;
  int rc = 0;
  if ((rc = ensure_host_buffers(e, w, d.L.total, n))) return rc;      // (a no-op: submit_host_batch has grown every slot's staging)
  if (d.cap) w.cb.L = cap_layout(n, d.cap->P, d.cap->G, d.cap->dev_blob_cap());
  if (d.cap && (rc = ensure_capture_buffers(e, w.cb, w.cb.L, d.cap->needs_work))) return rc;
  if (d.cap && d.cap->org && (rc = ensure_origin_buffers(e, w.ob, (size_t)n * d.cap->G, d.cap->origin_launch()))) return rc;
  if (d.capmix) w.cb.L = cap_layout_sized(d.capmix->plan.shape.J, d.capmix->plan.shape.Gt, d.capmix->out->cap_blob_cap);
  if (d.capmix && (rc = ensure_capture_buffers(e, w.cb, w.cb.L, d.capmix->needs_work))) return rc;
  if (d.capmix && d.capmix->org && (rc = ensure_origin_buffers(e, w.ob, d.capmix->plan.shape.Gt, d.capmix->origin_launch()))) return rc;
  if (d.scan && (rc = ensure_scan_buffers(e, w.sb, n, d.scan->max_sigs, d.scan->out->sel_blob_cap))) return rc;
  if (d.keyrec && (rc = ensure_keyrec_buffers(e, w.kb, n, (size_t)(d.sel ? d.key_total : d.raw_total), d.sel != nullptr))) return rc;
  if (d.body && (rc = ensure_body_buffers(e, w.bb, n, (size_t)d.raw_total))) return rc;
  if (d.enc && !d.enc->device_plan && (rc = ensure_encode_buffers(e, w.eb, n, d.enc->plan.total, 0))) return rc;
  if (d.enc && d.enc->device_plan && (rc = ensure_encode_buffers_planned(e, w.eb, n, d.enc->bytes_cap))) return rc;
  return 0;
}

// 2. The image in the slot's pinned buffer.  The gathered shape: the CSR arrays are written where they will be read from (prefix sums over
// the lengths), and every e-mail's three buffers go to their places in the blobs — the pool takes runs of consecutive e-mails (CopyPool::gather).
void pack_gathered(zke_engine* e, Slot& w, const HostBatch& d, uint8_t* hp) {
  const uint32_t n = d.b.n;
  const ImageLayout& L = d.L;
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
}
// The packed shape: the offsets are copied as they are (the kernels subtract off[0] themselves and the device pointers of
// device_view are biased by -off[0]): nothing is rebased, nothing is allocated, every byte is written once.
void pack_packed(zke_engine* e, const HostBatch& d, uint8_t* hp) {
  const uint32_t n = d.b.n;
  const ImageLayout& L = d.L;
  CopyPool::Piece pc[8] = {
      {hp + L.raw_off, d.b.raw_off, (size_t)(n + 1) * 8}, {hp + L.dom_off, d.b.domain_off, (size_t)(n + 1) * 8},
      {hp + L.key_off, d.b.key_off, (size_t)(n + 1) * 8}, {hp + L.key_type, d.b.key_type, n},
      {hp + L.ext_null, d.b.ext_null, d.b.ext_null ? n : 0u}, {hp + L.raw, d.b.raw_blob + d.raw_base, (size_t)d.raw_total},
      {hp + L.dom, d.b.domain_blob + d.dom_base, (size_t)d.dom_total}, {hp + L.key, d.b.key_blob + d.key_base, (size_t)d.key_total}};
  if (e->pool) e->pool->copy(pc, 8);
  else for (const auto& p : pc) if (p.n) stage_copy(p.dst, p.src, p.n);
}
// Either shape, then the capture tables of a regex batch (small) and the plan sections: they ride in the same image, the batch is
// still ONE copy.
void pack_image(zke_engine* e, Slot& w, const HostBatch& d) {
  uint8_t* hp = w.h_image.as<uint8_t>();
  const ImageLayout& L = d.L;
  if (d.refs) pack_gathered(e, w, d, hp);
  else pack_packed(e, d, hp);
  if (d.cap_words) {
    stage_copy(hp + L.cap_off, d.b.cap_off, d.cap_words * 4);
    stage_copy(hp + L.cap_str_off, d.b.cap_str_off, d.cap_strs * 4);
    stage_copy(hp + L.cap_blob, d.b.cap_blob, d.cap_bytes);
  }
  uint8_t* sp = hp + L.mixed;
  if (d.mixed) stage_mixed(sp, d.S.mixed, d.mixed->plan);
  if (d.capmix) stage_capmix(sp + d.S.capmix_at, d.S.capmix, d.capmix->plan, d.capmix->part);
  if (d.enc) stage_enc(sp + d.S.enc_at, d.S.enc, d.enc->plan, d.enc->device_plan, d.enc->ext_off, d.b.n, d.enc->ext_str_off, d.enc->ext_blob);
}

// 3. ONE H2D of the image.
int upload_image(zke_engine* e, Slot& w, size_t bytes, hipStream_t s) {
  if (ZKE_HOST_COPY_STREAM && bytes >= (256u << 10)) {
    // The image crosses PCIe on one of the engine's TWO copy streams, taken in turn, and the slot's stream waits for it.  Issued
    // on the slots' own 22 streams the input copies moved 31 GB/s in aggregate — one DMA engine's rate —, on one copy stream the
    // same; on two, 48 GB/s = 84 % of the link (122 us per 1 024-e-mail batch instead of 186; three streams: 141 us, four: worse).
    // Nothing on the device has to be waited for first: the slot's previous host batch — the only earlier user of d_image — was
    // retired on the host before the image was packed.  (Small images stay on the slot's stream: the cross-stream event costs a
    // single e-mail 16 us of latency and buys nothing.)
    std::lock_guard<std::mutex> cg(e->copy_mu);
    hipStream_t cs = e->copy_stream[e->copy_turn++ % ZKE_COPY_STREAMS];
    HIPCHK(e, hipMemcpyAsync(w.d_image.p, w.h_image.p, bytes, hipMemcpyHostToDevice, cs));
    HIPCHK(e, hipEventRecord(w.h2d_done, cs));
    HIPCHK(e, hipStreamWaitEvent(s, w.h2d_done, 0));
  } else {
    HIPCHK(e, hipMemcpyAsync(w.d_image.p, w.h_image.p, bytes, hipMemcpyHostToDevice, s));
  }
  return 0;
}

// 4. The batch as the kernels see it: the descriptor with its pointers into the slot's image in HBM.
zke_batch device_view(const Slot& w, const HostBatch& d) {
  const ImageLayout& L = d.L;
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
  return dv;
}

// 5. The launches.  A batch that is ONE stand-alone side launch instead of the verify pipeline (its twin's copy back is the launch's own) ...
bool side_launch_alone(const HostBatch& d) { return d.scan || d.body || (d.keyrec && !d.sel); }
// ... or the pipeline: behind the key-record prefix if the keys come as records, the plan sections viewed in HBM, the encode launches behind it.
int launch_verify(zke_engine* e, Slot& w, const HostBatch& d, zke_batch& dv, bool want_em, bool want_clean, hipStream_t s) {
  const uint32_t n = d.b.n;
  int rc = 0;
  uint64_t key_hint = d.key_total;
  if (d.keyrec) {
    if ((rc = launch_keyrec_prefix(e, w.kb, dv, d.keyrec->mode, s))) return rc;
    // (run_device_pipeline reads "the keys average more than an RSA-2048 key's 270 bytes" from the total: a 2048-bit
    // SubjectPublicKeyInfo record is about 410 characters, a 3072-bit one 580)
    key_hint = d.key_total > (uint64_t)n * 480 ? (uint64_t)n * 273 : 0;
  }
  const uint8_t* sp = w.d_image.as<uint8_t>() + d.L.mixed;      // the plan sections, as pack_image staged them
  const MixedLaunch ml = mixed_view(sp, d.S.mixed, d.mixed ? &d.mixed->plan : nullptr);
  const CapMixedLaunch cl{d.capmix ? d.capmix->plan.shape.J : 0u, d.capmix ? d.capmix->plan.shape.Gt : 0u, d.capmix && d.capmix->needs_work,
                          d.capmix && d.capmix->origin_launch(), capmix_view(sp + d.S.capmix_at, d.S.capmix, ml.job_off)};
  EncodeArgs ea = enc_view(sp + d.S.enc_at, d.S.enc);
  const bool planned = d.enc && d.enc->device_plan;
  LossyLaunch ll{};
  if (planned)             // the gather launch of this extraction also plans the encoding: where it reads the external inputs, where the jobs go
    ll = LossyLaunch{d.enc->plan.ext_strs ? reinterpret_cast<const uint32_t*>(ea.jobs) : nullptr, ea.ext_str_off,
                     reinterpret_cast<EncodeJob*>(w.eb.t.d.as<uint8_t>() + w.eb.jobs_at), d.enc->bytes_cap};
  if ((rc = run_device_pipeline(e, w, &dv, d.raw_total, key_hint, w.d_results.as<zke_result>(), s, want_em, batch_clock(e), want_clean, d.cap,
                                d.mixed ? &ml : nullptr, d.capmix ? &cl : nullptr, planned ? &ll : nullptr))) return rc;
  if (!d.enc) return 0;
  // the encodings of the records just written and their digests, two more launches on the same stream
  ea.records = w.d_results.as<zke_result>();
  ea.match_str_off = dv.cap_str_off; ea.match_blob = dv.cap_blob;
  if (planned) {           // the jobs are the gather launch's, the matches the tables it has just written in the slot's capture buffer
    ea.jobs = ll.jobs;
    ea.match_str_off = reinterpret_cast<const uint32_t*>(w.cb.t.d.as<uint8_t>() + w.cb.L.cap_str_off);
    ea.match_blob = w.cb.t.d.as<uint8_t>() + w.cb.L.blob;
  }
  return launch_encode(e, w.eb, ea, s, planned);
}
int launch_host_batch(zke_engine* e, Slot& w, const HostBatch& d, zke_batch& dv, bool want_em, bool want_clean, StageTimer& tm, hipStream_t s) {
  if (d.scan) return launch_scan(e, w.sb, dv, batch_clock(e), tm, s);
  if (d.body) return launch_body(e, w.bb, dv, d.body->flags, tm, s);
  if (d.keyrec && !d.sel) return launch_keyrec(e, w.kb, dv, d.keyrec->mode, tm, s);
  return launch_verify(e, w, d, dv, want_em, want_clean, s);
}

// 6. The D2H of every twin still in HBM (behind the pipeline: records, encodings, key records; captures, origins), the event, the debt.
int fetch_and_file(zke_engine* e, Slot& w, const HostBatch& d, zke_result* out, StageTimer& tm, hipStream_t s) {
  if (!side_launch_alone(d)) {
    const bool planned = d.enc && d.enc->device_plan;
    HIPCHK(e, hipMemcpyAsync(w.h_results.p, w.d_results.p, (size_t)d.b.n * sizeof(zke_result), hipMemcpyDeviceToHost, s));
    if (d.enc) HIPCHK(e, w.eb.t.fetch(planned ? w.eb.L.bytes : w.eb.L.prefix, s));
    if (d.keyrec) HIPCHK(e, w.kb.t.fetch(w.kb.L.total, s));
  }
  if (d.cap || d.capmix) HIPCHK(e, w.cb.t.fetch(w.cb.L.fixed_end, s));
  if (((d.cap && d.cap->org) || (d.capmix && d.capmix->org)) && w.ob.launched) HIPCHK(e, w.ob.t.fetch(w.ob.L.total, s));
  tm.mark(MK_D2H);
  HIPCHK(e, hipEventRecord(w.host_done, s));
  w.host_gen++;
  w.owed = pending_delivery(d, out);
  return 0;
}

// One host batch into slot w (caller holds its lock): the stages above in order.  The slot's use ends on every way out (SlotUse).
int submit_host(zke_engine* e, Slot& w, const HostBatch& d, zke_result* out, bool want_em, bool want_clean) {
  if (int rc = retire_host(e, w)) return rc;         // the pinned buffers are about to be overwritten
  if (int rc = ensure_output_buffers(e, w, d)) return rc;
  pack_image(e, w, d);
  hipStream_t s = w.stream;
  SlotUse use(e, w, s);
  if (int rc = use.acquire()) return rc;
  StageTimer tm(e, &w, s);
  tm.mark(MK_START);
  if (int rc = upload_image(e, w, d.L.total, s)) return rc;
  tm.mark(MK_H2D);
  zke_batch dv = device_view(w, d);
  if (int rc = launch_host_batch(e, w, d, dv, want_em, want_clean, tm, s)) return rc;
  if (int rc = fetch_and_file(e, w, d, out, tm, s)) return rc;
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
  if (d.capmix && n) capmix_resolve(e, *d.capmix);   // likewise the part table of a mixed extraction
  if (d.mixed && n) if (int r = mixed_resolve(e, *d.mixed)) return r;      // likewise the DFA pairs' tables a mixed batch's segments point to
  uint32_t slot;
  uint64_t t;
  Slot& w = next_slot(e, slot, &t);
  // A batch nobody waited for is delivered once as many batches as the engine has slots have been submitted behind it.  While tickets went
  // round the slots that was the slot's own turn; ordered by queue, a slot on a fuller queue comes round later than that, so the batch of
  // ticket t - slots is delivered here — the wait every submission has always made.  (Before this slot's lock is taken, never under it.)
  const uint64_t S = e->slots.size();
  if (e->order.n_queues && t >= S) {
    const uint32_t due = slot_for_ticket(e->order, t - S);
    if (due != slot) { Slot& o = *e->slots[due]; std::lock_guard<std::mutex> go(o.mu); if (int r = retire_host(e, o)) return r; }
  }
  std::lock_guard<std::mutex> g(w.mu);
  if (!n) { *ticket = make_ticket(slot, w.host_retired); return 0; }      // nothing to wait for
  if (int r = submit_host(e, w, d, out, dbg && dbg->em, dbg && dbg->clean_body)) return r;
  if (ticket) { *ticket = make_ticket(slot, w.host_gen); return 0; }
  int cap_rc = 0;
  if (int r = retire_host(e, w, &cap_rc)) return r;
  if (cap_rc) return cap_rc;
  return dbg ? copy_debug_out(e, w, d.b, out, dbg) : 0;
}

// A synchronous entry: its asynchronous one (`submit`, given the ticket), then the wait for the ticket — an empty batch has none.
template <class Submit> int submit_and_wait(zke_engine* e, uint32_t n, Submit submit) {
  uint64_t ticket = 0;
  if (int r = submit(&ticket)) return r;
  return n ? zke_batch_wait(e, ticket) : 0;
}

// ---- key selection (zke_select_keys, zke_select_keys_from_records)
// cand_off of a selection over n e-mails, checked: M candidates in all, the first of them candidate `base` of the caller's list
int selection_shape(const char* who, const uint32_t* cand_off, uint32_t n, uint32_t& base, uint32_t& M) {
  if (n && !rising(cand_off, n)) return arg_error(who, "cand_off is not non-decreasing");
  base = n ? cand_off[0] : 0;
  M = n ? cand_off[n] - base : 0;
  return 0;
}
// ONE batch of the (e-mail, candidate) pairs: the raw e-mail and the domain by reference, once per candidate; key_of(k, m) puts
// candidate k's key (or, with `keyrec`, its record: the image's key section then holds records) into the pair m.  The pending
// delivery folds the pairs' records per e-mail.
template <class KeyOf> int submit_selection(zke_engine* e, const char* who, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off, uint32_t M,
                                            zke_result* out, uint32_t* chosen, const KeyrecReq* keyrec, uint64_t* ticket, KeyOf key_of) {
  std::vector<zke_email_ref> refs(M);
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t k = cand_off[i]; k < cand_off[i + 1]; k++) {
      zke_email_ref& m = refs[k - cand_off[0]];
      m = emails[i];
      key_of(k, m);
    }
  HostBatch d;
  if (int r = host_batch(d, who, out, refs.data(), M, nullptr)) return r;
  const SelectReq q{cand_off, n, out, chosen};
  if (M) { d.sel = &q; d.keyrec = keyrec; }
  else if (n) fold_selection(nullptr, std::vector<uint32_t>((size_t)n + 1, 0u), out, chosen);      // no candidate anywhere: nothing to run
  return submit_host_batch(e, d, out, ticket);
}

}  // namespace

extern "C" {

int zke_engine_reserve_host(zke_engine* e, uint32_t max_n, uint64_t max_input_bytes) {
  if (!e) return ZKE_E_ARG;
  // offsets, key types and 64-byte alignment on top of the blobs (image_layout)
  const size_t image = (size_t)max_input_bytes + (size_t)(max_n + 1) * 24 + 2 * (size_t)max_n + 16 * 64 + 4 * 64;
  if (image <= e->host_image_cap.load() && max_n <= e->host_n_cap.load()) return 0;
  return grow_host_staging(e, image, max_n);
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

// `&[EmailWithRegex]` with a RegexInfo per value (include/zkemail_amd.h): the checks and the sizes here, before anything is staged;
// the plan once the registry can be read (mixed_resolve); its tables in the slot's image (submit_host).
namespace {
// What a mixed verify and a mixed extraction check of their configs before they look at one: the count and the two arrays.
int check_mixed_configs(const char* who, uint32_t n_configs, const void* configs, const uint32_t* config_of, uint32_t n) {
  if (n_configs > ZKE_MIXED_MAX_CONFIGS) return arg_error(who, "more than ZKE_MIXED_MAX_CONFIGS configs");
  if ((n_configs && !configs) || (n && !config_of)) return arg_error(who, "null pointer");
  return 0;
}
// The request of a mixed batch from the caller's zke_regex_mixed: the checks that need no registry, the configs' part counts, the shape.
int mixed_request(const char* who, const zke_regex_mixed* mixed, uint32_t n, MixedReq& q) {
  if (int r = check_mixed_configs(who, mixed->n_configs, mixed->configs, mixed->config_of, n)) return r;
  q.in = mixed; q.n = n;
  q.counts.resize(mixed->n_configs);
  for (uint32_t c = 0; c < mixed->n_configs; c++) {
    const zke_regex_config& cf = mixed->configs[c];
    if ((cf.n_header_parts && !cf.header_part_ids) || (cf.n_body_parts && !cf.body_part_ids)) return arg_error(who, "part-id list is null");
    q.counts[c] = MixedConfigIn{cf.n_header_parts, cf.n_body_parts};
  }
  if (const char* why = mixed_plan_check(mixed->config_of, n, q.counts.data(), mixed->n_configs, q.shape)) return arg_error(who, why);
  return 0;
}
}  // namespace

int zke_verify_emails_mixed_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_mixed* mixed, zke_result* out,
                                  uint64_t* ticket) {
  static const char who[] = "zke_verify_emails_mixed";
  if (!e) return ZKE_E_ARG;
  if (!mixed || !ticket) return arg_error(who, "null pointer");
  MixedReq q;
  if (int r = mixed_request(who, mixed, n, q)) return r;
  HostBatch d;
  if (int r = host_batch(d, who, out, emails, n, nullptr, &q)) return r;
  return submit_host_batch(e, d, out, ticket);
}

int zke_verify_emails_mixed(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_mixed* mixed, zke_result* out) {
  return submit_and_wait(e, n, [&](uint64_t* t) { return zke_verify_emails_mixed_async(e, emails, n, mixed, out, t); });
}

int zke_verify_emails_with_regex(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_lists* lists, zke_result* out) {
  return submit_and_wait(e, n, [&](uint64_t* t) { return zke_verify_emails_with_regex_async(e, emails, n, lists, out, t); });
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
  if (out->scan_status_cap < out->scan_status_need || out->sig_off_cap < out->sig_off_need) return nomem_error(who, "a zke_sig_scan buffer is smaller than its *_need");
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
  return submit_and_wait(e, n, [&](uint64_t* t) { return zke_scan_signatures_async(e, emails, n, max_sigs, out, t); });
}

int zke_select_keys_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off, const zke_key_ref* keys,
                          zke_result* out, uint32_t* chosen, uint64_t* ticket) {
  static const char who[] = "zke_select_keys";
  if (!e) return ZKE_E_ARG;
  if (!ticket || (n && (!emails || !cand_off || !out || !chosen))) return arg_error(who, "null pointer");
  uint32_t base = 0, M = 0;
  if (int r = selection_shape(who, cand_off, n, base, M)) return r;
  if (M >> 31) return arg_error(who, "2^31 candidates or more");
  if (M && !keys) return arg_error(who, "null pointer");
  return submit_selection(e, who, emails, n, cand_off, M, out, chosen, nullptr, ticket,
                          [&](uint32_t k, zke_email_ref& m) { m.key = keys[k].key; m.key_len = keys[k].key_len; m.key_type = keys[k].key_type; });
}

int zke_select_keys(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off, const zke_key_ref* keys,
                    zke_result* out, uint32_t* chosen) {
  return submit_and_wait(e, n, [&](uint64_t* t) { return zke_select_keys_async(e, emails, n, cand_off, keys, out, chosen, t); });
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
  if (out->infos_cap < m) return nomem_error(who, "zke_keyrec_out.infos is smaller than infos_need");
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
  return submit_and_wait(e, m, [&](uint64_t* t) { return zke_decode_key_records_async(e, recs, m, mode, out, t); });
}

int zke_select_keys_from_records_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off,
                                       const zke_keyrec_ref* recs, uint32_t mode, zke_result* out, uint32_t* chosen,
                                       zke_keyrec_out* keys_out, uint64_t* ticket) {
  static const char who[] = "zke_select_keys_from_records";
  if (!e) return ZKE_E_ARG;
  if (!ticket || !keys_out || (n && (!emails || !cand_off || !out || !chosen))) return arg_error(who, "null pointer");
  uint32_t base = 0, M = 0;
  if (int r = selection_shape(who, cand_off, n, base, M)) return r;
  if (int r = keyrec_args(who, recs ? recs + base : nullptr, M, mode, keys_out)) return r;
  const KeyrecReq kq{mode, keys_out};
  return submit_selection(e, who, emails, n, cand_off, M, out, chosen, &kq, ticket,
                          [&](uint32_t k, zke_email_ref& m) { m.key = recs[k].txt; m.key_len = keyrec_staged(recs[k].len); m.key_type = ZKE_KEY_RSA; });
}

int zke_select_keys_from_records(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off,
                                 const zke_keyrec_ref* recs, uint32_t mode, zke_result* out, uint32_t* chosen, zke_keyrec_out* keys_out) {
  return submit_and_wait(e, n, [&](uint64_t* t) { return zke_select_keys_from_records_async(e, emails, n, cand_off, recs, mode, out, chosen, keys_out, t); });
}

// ---- extract_email_body for whole batches (include/zkemail_amd.h; kernel: bodyext.hip.h)
int zke_extract_bodies_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, uint32_t flags, zke_body_out* out, uint64_t* ticket) {
  static const char who[] = "zke_extract_bodies";
  if (!e) return ZKE_E_ARG;
  if (!ticket || !out || (n && !emails)) return arg_error(who, "null pointer");
  if (flags & ~ZKE_BODYF_PART_KEEPS_EOL) return arg_error(who, "unknown flag bits");
  for (uint32_t i = 0; i < n; i++) {
    if (emails[i].raw_len && !emails[i].raw) return arg_error(who, "null buffer with a length");
    if (emails[i].raw_len >= (1ull << 31)) return arg_error(who, "an e-mail of 2^31 bytes or more");
  }
  out->infos_need = n; out->bytes_need = 0;
  if (out->infos_cap < n) return nomem_error(who, "zke_body_out.infos is smaller than infos_need");
  if ((n && !out->infos) || (out->bytes_cap && !out->bytes)) return arg_error(who, "null buffer in zke_body_out");
  std::vector<zke_email_ref> refs(n);                 // only the raw e-mails travel: no domains, no keys
  for (uint32_t i = 0; i < n; i++) { refs[i] = zke_email_ref{}; refs[i].raw = emails[i].raw; refs[i].raw_len = emails[i].raw_len; }
  HostBatch d;
  if (int r = host_batch(d, who, reinterpret_cast<const zke_result*>(out), refs.data(), n, nullptr)) return r;
  const BodyReq q{flags, out};
  d.body = &q;
  return submit_host_batch(e, d, nullptr, ticket);
}

int zke_extract_bodies(zke_engine* e, const zke_email_ref* emails, uint32_t n, uint32_t flags, zke_body_out* out) {
  return submit_and_wait(e, n, [&](uint64_t* t) { return zke_extract_bodies_async(e, emails, n, flags, out, t); });
}

// ---- the verifier outputs encoded on the device (include/zkemail_amd.h; plan: encode_plan.hip.h, kernel: encode.hip.h)
namespace {
// `enc` against a plan's sizes, which are exact: the needs written back, ZKE_E_NOMEM when either buffer is too small
int check_encoded_out(zke_encoded_out* o, uint32_t n, uint64_t total, const char* who) {
  o->infos_need = n; o->bytes_need = (size_t)total;
  if (o->infos_cap < n || o->bytes_cap < total) return nomem_error(who, "a zke_encoded_out buffer is smaller than its *_need");
  if ((n && !o->infos) || (total && !o->bytes)) return arg_error(who, "null buffer in zke_encoded_out");
  return 0;
}
}  // namespace

// The entry `in` chooses, checked and measured as that entry does it; then the plan over the tables just checked — kinds, places, the
// exact sizes — and `enc` against it: all of it before anything is staged.
int zke_verify_emails_encoded_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_encode_in* in, zke_result* out,
                                    zke_encoded_out* enc, uint64_t* ticket) {
  static const char who[] = "zke_verify_emails_encoded";
  if (!e) return ZKE_E_ARG;
  if (!ticket || !enc) return arg_error(who, "null pointer");
  const zke_encode_in none{};
  if (!in) in = &none;
  if (const char* why = encode_lists_check(in->lists, in->mixed)) return arg_error(who, why);
  MixedReq mq;
  if (in->mixed) if (int r = mixed_request(who, in->mixed, n, mq)) return r;
  HostBatch d;
  if (int r = host_batch(d, who, out, emails, n, in->lists, in->mixed ? &mq : nullptr, nullptr, false)) return r;
  std::vector<uint32_t> kinds(n, in->lists ? ENC_KIND_WITH_REGEX : ENC_KIND_EMAIL), row_off;
  EncodeTables t;
  t.ext_off = in->ext_off; t.ext_str_off = in->ext_str_off; t.ext_blob = in->ext_blob;
  t.match_off = d.b.cap_off; t.match_str_off = d.b.cap_str_off; t.match_blob = d.b.cap_blob;      // (null where no string is named: measure_host_batch)
  if (in->lists) t.row_stride = in->lists->n_header_parts + in->lists->n_body_parts;
  if (in->mixed) {         // a mixed batch's rows are its jobs: job_off, the prefix sum of the configs' part counts
    row_off.resize((size_t)n + 1);
    uint32_t j = 0;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t c = in->mixed->config_of[i];
      row_off[i] = j;
      if (c == ZKE_CONFIG_NONE) continue;
      kinds[i] = ENC_KIND_WITH_REGEX;
      j += mq.counts[c].n_header_parts + mq.counts[c].n_body_parts;
    }
    row_off[n] = j;
    t.row_off = row_off.data();
  }
  EncodeReq q;
  q.out = enc; q.ext_str_off = in->ext_str_off; q.ext_blob = in->ext_blob;
  if (const char* why = encode_plan_build(n, kinds.data(), t, q.plan)) return arg_error(who, why);
  if (int r = check_encoded_out(enc, n, q.plan.total, who)) return r;
  d.enc = &q;
  layout_host_batch(d);
  return submit_host_batch(e, d, out, ticket);
}

int zke_verify_emails_encoded(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_encode_in* in, zke_result* out,
                              zke_encoded_out* enc) {
  return submit_and_wait(e, n, [&](uint64_t* t) { return zke_verify_emails_encoded_async(e, emails, n, in, out, enc, t); });
}

namespace {
// the sizes an extraction over n e-mails needs, written back; ZKE_E_NOMEM when a buffer of known size is too small
// (NP jobs and NG columns: n * P and n * G of one part list per batch, J and Gt of a mixed extraction)
int check_capture_out_sized(zke_capture_out* o, size_t NP, size_t NG, const char* who) {
  if (!o) return arg_error(who, "null zke_capture_out");
  o->spans_need = NG * 2; o->flags_need = NG; o->cap_off_need = NP + 1; o->cap_str_off_need = NG + 1;
  o->cap_blob_need = 0; o->n_strings = 0;
  // string offsets are 32-bit, as the verify entry's tables are: what n * G spans of ZKE_CAP_MAX_SPAN bytes could not address is refused
  if ((uint64_t)NG * ZKE_CAP_MAX_SPAN > 0xFFFFFFFFull) return arg_error(who, "n x groups beyond what 32-bit string offsets address (n * G * ZKE_CAP_MAX_SPAN must stay below 4 GiB): split the batch");
  if (o->spans_cap < o->spans_need || o->flags_cap < o->flags_need || o->cap_off_cap < o->cap_off_need || o->cap_str_off_cap < o->cap_str_off_need)
    return nomem_error(who, "a zke_capture_out buffer is smaller than its *_need");
  if (!o->spans || !o->flags || !o->cap_off || !o->cap_str_off || (o->cap_blob_cap && !o->cap_blob)) return arg_error(who, "null buffer in zke_capture_out");
  return 0;
}
int check_capture_out(zke_capture_out* o, uint32_t n, uint32_t P, uint32_t G, const char* who) { return check_capture_out_sized(o, (size_t)n * P, (size_t)n * G, who); }
// the same for the origins of a mapped extraction: both sizes are known up front
int check_capture_origin_sized(zke_capture_origin* o, size_t NG, const char* who) {
  if (!o) return arg_error(who, "null zke_capture_origin");
  o->spans_need = NG * 2; o->flags_need = NG;
  if (o->spans_cap < o->spans_need || o->flags_cap < o->flags_need) return nomem_error(who, "a zke_capture_origin buffer is smaller than its *_need");
  if (NG && (!o->spans || !o->flags)) return arg_error(who, "null buffer in zke_capture_origin");
  return 0;
}
int check_capture_origin(zke_capture_origin* o, uint32_t n, uint32_t G, const char* who) { return check_capture_origin_sized(o, (size_t)n * G, who); }

// The request of an extraction over one pair of part lists (non-null where they have entries): the parts' shapes, no registry
// involved.  `lossy`: the gather launch repairs the strings and plans the encoding (zke_extract_captures_encoded).
int capture_request(CaptureReq& q, const zke_capture_part* header_parts, uint32_t n_header_parts, const zke_capture_part* body_parts,
                    uint32_t n_body_parts, zke_capture_out* caps, bool lossy, const char* who) {
  const uint32_t P = n_header_parts + n_body_parts;
  if (P == 0 || P > ZKE_CAP_MAX_PARTS || n_header_parts > ZKE_CAP_MAX_PARTS) return arg_error(who, "1 .. ZKE_CAP_MAX_PARTS parts");
  q.P = P; q.n_header_parts = n_header_parts; q.out = caps; q.lossy = lossy;
  q.dfa_ids.resize(P);
  for (uint32_t p = 0; p < P; p++) {
    const zke_capture_part& cp = p < n_header_parts ? header_parts[p] : body_parts[p - n_header_parts];
    q.dfa_ids[p] = cp.dfa_id;
    if (int r = capture_part_shape(q, p, cp.prog_id, cp.groups, cp.n_groups, who)) return r;
  }
  return 0;
}

// zke_extract_captures_async and its mapped form (`mapped`: org is wanted, and checked behind caps)
int extract_captures_submit(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                            uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                            zke_capture_out* caps, bool mapped, zke_capture_origin* org, uint64_t* ticket, const char* who) {
  if (!e) return ZKE_E_ARG;
  if (!ticket || !caps || (mapped && !org) || (n_header_parts && !header_parts) || (n_body_parts && !body_parts)) return arg_error(who, "null pointer");
  CaptureReq q;
  if (int r = capture_request(q, header_parts, n_header_parts, body_parts, n_body_parts, caps, false, who)) return r;
  if (int r = check_capture_out(caps, n, q.P, q.G, who)) return r;
  if (mapped) { if (int r = check_capture_origin(org, n, q.G, who)) return r; q.org = org; }
  zke_regex_lists lists{n_header_parts, q.dfa_ids.data(), n_body_parts, q.dfa_ids.data() + n_header_parts, nullptr, nullptr, nullptr};
  HostBatch d;
  if (int r = host_batch(d, who, out, emails, n, &lists)) return r;
  d.cap = &q;
  return submit_host_batch(e, d, out, ticket);
}
}  // namespace

int zke_extract_captures_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                               uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                               zke_capture_out* caps, uint64_t* ticket) {
  return extract_captures_submit(e, emails, n, header_parts, n_header_parts, body_parts, n_body_parts, out, caps, false, nullptr, ticket,
                                 "zke_extract_captures");
}

int zke_extract_captures(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                         uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                         zke_capture_out* caps) {
  return submit_and_wait(e, n, [&](uint64_t* t) {
    return zke_extract_captures_async(e, emails, n, header_parts, n_header_parts, body_parts, n_body_parts, out, caps, t);
  });
}

int zke_extract_captures_mapped_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                                      uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                                      zke_capture_out* caps, zke_capture_origin* org, uint64_t* ticket) {
  return extract_captures_submit(e, emails, n, header_parts, n_header_parts, body_parts, n_body_parts, out, caps, true, org, ticket,
                                 "zke_extract_captures_mapped");
}

int zke_extract_captures_mapped(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                                uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                                zke_capture_out* caps, zke_capture_origin* org) {
  return submit_and_wait(e, n, [&](uint64_t* t) {
    return zke_extract_captures_mapped_async(e, emails, n, header_parts, n_header_parts, body_parts, n_body_parts, out, caps, org, t);
  });
}

// ---- extraction, UTF-8 repair and encoding in one batch (include/zkemail_amd.h; kernels: capture_lossy.hip.h, encode.hip.h).  The
// extraction's request with the lossy gather launch, and an encoding whose plan is the device's: what can be refused is refused
// here, from the part lists and the external-input table alone, before anything is staged.
int zke_extract_captures_encoded_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                                       uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                                       zke_capture_out* caps, const uint32_t* ext_off, const uint32_t* ext_str_off, const uint8_t* ext_blob,
                                       zke_encoded_out* enc, uint64_t* ticket) {
  static const char who[] = "zke_extract_captures_encoded";
  if (!e) return ZKE_E_ARG;
  if (!ticket || !enc || (n_header_parts && !header_parts) || (n_body_parts && !body_parts)) return arg_error(who, "null pointer");
  CaptureReq q;
  if (int r = capture_request(q, header_parts, n_header_parts, body_parts, n_body_parts, caps, true, who)) return r;
  // a repaired string is at most three times its span: what n * G of those could not address in 32 bits is refused
  const uint64_t str_worst = 3ull * ZKE_CAP_MAX_SPAN, blob_worst = (uint64_t)n * q.G * str_worst;
  if (blob_worst > 0xFFFFFFFFull) return arg_error(who, "n x groups beyond what 32-bit string offsets address (n * G * 3 * ZKE_CAP_MAX_SPAN must stay below 4 GiB): split the batch");
  if (caps) if (int r = check_capture_out(caps, n, q.P, q.G, who)) return r;
  EncodeReq eq;
  eq.device_plan = true; eq.n = n; eq.out = enc; eq.ext_off = ext_off; eq.ext_str_off = ext_str_off; eq.ext_blob = ext_blob;
  if (const char* why = encode_table_check(ext_off, n, ext_str_off, ext_blob, eq.plan.ext_strs, eq.plan.ext_bytes)) return arg_error(who, why);
  // the largest matches array the part lists can yield, and with it the largest encoding of every e-mail
  const uint64_t match_worst = 32 + (uint64_t)q.G * (64 + str_worst);
  uint64_t bytes_worst = 0;
  for (uint32_t i = 0; i < n; i++) {
    uint64_t size = 32 + 96 + 64;
    if (!enc_add_array(ext_str_off, eq.plan.ext_strs ? ext_off[i] : 0u, eq.plan.ext_strs ? ext_off[i + 1] : 0u, size) || size + match_worst >= ENC_MAX_LEN)
      return arg_error(who, "an encoding could reach 2^32 bytes (the external inputs and the largest matches the part lists can yield)");
    bytes_worst += size + match_worst;
  }
  enc->infos_need = n; enc->bytes_need = 0;
  if (enc->infos_cap < n) return nomem_error(who, "zke_encoded_out.infos is smaller than infos_need");
  if ((n && !enc->infos) || (enc->bytes_cap && !enc->bytes)) return arg_error(who, "null buffer in zke_encoded_out");
  eq.bytes_cap = std::min<uint64_t>(enc->bytes_cap, bytes_worst);
  zke_regex_lists lists{n_header_parts, q.dfa_ids.data(), n_body_parts, q.dfa_ids.data() + n_header_parts, nullptr, nullptr, nullptr};
  HostBatch d;
  if (int r = host_batch(d, who, out, emails, n, &lists, nullptr, nullptr, false)) return r;
  // the strings' blob on the device: the caller's capacity; without `caps`, what the strings cannot exceed (a group lies in a
  // canonical header or body, which is no longer than its e-mail but for a line end)
  q.lossy_blob_cap = (size_t)std::min<uint64_t>(blob_worst, caps ? (uint64_t)caps->cap_blob_cap : 3ull * q.G * (d.raw_total + 64ull * n));
  if (!n && caps) { caps->cap_off[0] = 0; caps->cap_str_off[0] = 0; }      // (nothing is launched: the empty tables are written here)
  d.cap = &q; d.enc = &eq;
  layout_host_batch(d);
  return submit_host_batch(e, d, out, ticket);
}

int zke_extract_captures_encoded(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                                 uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                                 zke_capture_out* caps, const uint32_t* ext_off, const uint32_t* ext_str_off, const uint8_t* ext_blob,
                                 zke_encoded_out* enc) {
  return submit_and_wait(e, n, [&](uint64_t* t) {
    return zke_extract_captures_encoded_async(e, emails, n, header_parts, n_header_parts, body_parts, n_body_parts, out, caps, ext_off,
                                              ext_str_off, ext_blob, enc, t);
  });
}

// ---- the extraction over `&[Email]` with a RegexConfig per e-mail (include/zkemail_amd.h): the checks, the plan's ragged half and the
// sizes here, before anything is staged; the programs and the DFA pairs once the registry can be read (capmix_resolve, mixed_resolve).
int zke_extract_captures_mixed_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_mixed* mixed, zke_result* out,
                                     zke_capture_out* caps, zke_capture_origin* org, uint64_t* ticket) {
  static const char who[] = "zke_extract_captures_mixed";
  if (!e) return ZKE_E_ARG;
  if (!mixed || !ticket || !caps) return arg_error(who, "null pointer");
  if (int r = check_mixed_configs(who, mixed->n_configs, mixed->configs, mixed->config_of, n)) return r;
  CapMixedReq q;
  q.out = caps; q.org = org;
  q.verify.counts.resize(mixed->n_configs);
  for (uint32_t c = 0; c < mixed->n_configs; c++) {
    const zke_capture_config& cf = mixed->configs[c];
    if (cf.n_header_parts > ZKE_CAP_MAX_PARTS || cf.n_body_parts > ZKE_CAP_MAX_PARTS - cf.n_header_parts || cf.n_header_parts + cf.n_body_parts == 0)
      return arg_error(who, "a config needs 1 .. ZKE_CAP_MAX_PARTS parts (ZKE_CONFIG_NONE is the way to say: no regex)");
    if ((cf.n_header_parts && !cf.header_parts) || (cf.n_body_parts && !cf.body_parts)) return arg_error(who, "part list is null");
    q.verify.counts[c] = MixedConfigIn{cf.n_header_parts, cf.n_body_parts};
    for (uint32_t p = 0; p < cf.n_header_parts + cf.n_body_parts; p++) {
      const zke_capture_part& cp = p < cf.n_header_parts ? cf.header_parts[p] : cf.body_parts[p - cf.n_header_parts];
      if (cp.n_groups > ZKE_CAP_MAX_GROUPS) return arg_error(who, "more than ZKE_CAP_MAX_GROUPS groups requested for a part");
      if (cp.n_groups && !cp.groups) return arg_error(who, "null group list");
      CapPartDev d{};
      d.code = ZKE_D_U_CAPTURE_PROGRAM;
      d.n_groups = cp.n_groups;
      for (uint32_t k = 0; k < cp.n_groups; k++) d.groups[k] = cp.groups[k];
      q.part.push_back(d);
      q.dfa_ids.push_back(cp.dfa_id); q.prog_ids.push_back(cp.prog_id); q.n_groups.push_back(cp.n_groups);
    }
  }
  if (const char* why = capmix_plan_build(mixed->config_of, n, q.verify.counts.data(), mixed->n_configs, q.n_groups.data(), q.plan)) return arg_error(who, why);
  for (size_t k = 0; k < q.part.size(); k++) q.part[k].gbase = q.plan.gbase[k];
  // the regex stage's half: zke_verify_emails_mixed's request over the same configs, without capture tables
  q.id_lists.resize(mixed->n_configs);
  for (uint32_t c = 0; c < mixed->n_configs; c++) {
    const uint32_t* ids = q.dfa_ids.data() + q.plan.cfgs[c].part0;
    q.id_lists[c] = zke_regex_config{q.verify.counts[c].n_header_parts, ids, q.verify.counts[c].n_body_parts, ids + q.verify.counts[c].n_header_parts};
  }
  q.lists = zke_regex_mixed{mixed->n_configs, q.id_lists.data(), mixed->config_of, nullptr, nullptr, nullptr};
  q.verify.in = &q.lists; q.verify.n = n;
  if (const char* why = mixed_plan_check(mixed->config_of, n, q.verify.counts.data(), mixed->n_configs, q.verify.shape)) return arg_error(who, why);
  HostBatch d;
  if (int r = host_batch(d, who, out, emails, n, nullptr, &q.verify, &q)) return r;
  if (int r = check_capture_out_sized(caps, q.plan.shape.J, q.plan.shape.Gt, who)) return r;
  if (org) if (int r = check_capture_origin_sized(org, q.plan.shape.Gt, who)) return r;
  if (!n) { caps->cap_off[0] = 0; caps->cap_str_off[0] = 0; }      // (nothing is launched: the empty tables are written here)
  return submit_host_batch(e, d, out, ticket);
}

int zke_extract_captures_mixed(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_mixed* mixed, zke_result* out,
                               zke_capture_out* caps, zke_capture_origin* org) {
  return submit_and_wait(e, n, [&](uint64_t* t) { return zke_extract_captures_mixed_async(e, emails, n, mixed, out, caps, org, t); });
}
}  // extern "C"
