// host_entry.hip.h — the entries whose batch lies in host memory: the batch descriptor and its checks, the packed image into a
// slot (host_stage.hip.h), upload, launches (pipeline.hip.h), delivery into the caller's buffers.  Stands for the reference's
// callers, `&[Email]` into verify_email / verify_email_with_regex (core/src/circuits.rs:9-68), and for what comes before a key is
// known: scan, key records, selection, captures.  Included by engine.hip behind pipeline.hip.h and registry.hip.h (one translation unit).
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
        const uint32_t id = p >= cf.n_header_parts ? cf.body_part_ids[p - cf.n_header_parts] : cf.header_part_ids[p];
        const RegisteredDfa* rd = id < e->dfas.size() ? e->dfas[id] : nullptr;
        PartInfo pi{};
        if (rd) { pi.detail = rd->detail; pi.lds_bytes = rd->lds_bytes; pi.idle = rd->idle; pi.dev = rd->valid ? rd->dev.as<RegexDev>() : nullptr; }
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

// A slot's buffers for one side output of a batch of n: the layout, then the buffers it asks for (ensure_side_buffers).
// `pack`: zke_select_keys_from_records, the decoded keys are packed for the front end.
int ensure_keyrec_buffers(zke_engine* e, KeyrecBufs& b, uint32_t m, size_t rec_total, bool pack) {
  b.L = keyrec_layout(m, rec_total);
  return ensure_side_buffers(e, b.t, b.L.total, b.L.total, pack ? &b.pack : nullptr, b.L.p_total, "key-record buffer allocation");
}
int ensure_body_buffers(zke_engine* e, BodyBufs& b, uint32_t n, size_t raw_total) {
  b.L = body_layout(n, raw_total);
  return ensure_side_buffers(e, b.t, b.L.total, b.L.total, &b.ovf, (size_t)n * HDR_OVF_BYTES, "body-extraction buffer allocation");
}
// `staged`: bytes of the building block's input (zke_encode_outputs), 0 where the batch's image carries it
int ensure_encode_buffers(zke_engine* e, EncBufs& b, uint32_t n, uint64_t blob, size_t staged) {
  b.L = enc_layout(n, blob);
  return ensure_side_buffers(e, b.t, b.L.total, b.L.prefix, staged ? &b.in : nullptr, staged, "output-encoding buffer allocation");
}
// a device-planned encoding: `cap` bytes of encodings, the jobs behind them, the infos alone pinned
int ensure_encode_buffers_planned(zke_engine* e, EncBufs& b, uint32_t n, uint64_t cap) {
  b.L = enc_layout_planned(n, cap, b.jobs_at);
  return ensure_side_buffers(e, b.t, b.L.total, b.L.bytes, nullptr, 0, "output-encoding buffer allocation");
}
// max_sigs record slots per e-mail and the caller's sel_blob_cap bytes of selectors (a selector is at most ZKE_MAX_TAGBUF bytes: a
// larger blob than that per record slot is never used)
int ensure_scan_buffers(zke_engine* e, ScanBufs& b, uint32_t n, uint32_t max_sigs, size_t sel_blob_cap) {
  b.L = scan_layout(n, max_sigs, std::min<size_t>(sel_blob_cap, (size_t)n * max_sigs * ZKE_MAX_TAGBUF));
  return ensure_side_buffers(e, b.t, b.L.total, b.L.total, &b.ovf, (size_t)n * HDR_OVF_BYTES, "signature-scan buffer allocation");
}
// `launched`: capture_origin_kernel runs for this batch; where it does not, nothing is allocated
int ensure_origin_buffers(zke_engine* e, OriginBufs& b, size_t NG, bool launched) {
  b.L = origin_layout_sized(NG);
  b.launched = launched;
  return b.launched ? ensure_side_buffers(e, b.t, b.L.total, b.L.total, nullptr, 0, "capture-origin buffer allocation") : 0;
}

// An extraction's tables from the slot's pinned twin (and the blob from HBM) into the caller's zke_capture_out.  Returns
// ZKE_E_NOMEM when the caller's cap_blob is too small for the strings (everything else is delivered; cap_blob_need says how much).
int deliver_captures(zke_engine* e, CapBufs& b, zke_capture_out* o, hipStream_t s) {
  const CapLayout& L = b.L;
  const uint8_t* hp = b.t.h.as<uint8_t>();
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
    HIPCHK(e, hipMemcpyAsync(o->cap_blob, b.t.d.as<uint8_t>() + L.blob, take, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  }
  if (bytes > L.blob_cap) return fail(e, ZKE_E_NOMEM, "capture extraction: cap_blob is smaller than the strings (zke_capture_out.cap_blob_need)");
  return 0;
}

// A mapped extraction's origins into the caller's zke_capture_origin: from the slot's pinned twin where capture_origin_kernel ran,
// else (no body part asks for a group) the spans themselves, which the capture buffer's pinned twin holds, and no flag.
void deliver_origins(const CapBufs& b, const OriginBufs& ob, zke_capture_origin* o) {
  const OriginLayout& L = ob.L;
  if (!L.NG) return;
  if (ob.launched) {
    const uint8_t* hp = ob.t.h.as<uint8_t>();
    memcpy(o->spans, hp, L.NG * 8);
    memcpy(o->flags, hp + L.flags, L.NG);
  } else {
    memcpy(o->spans, b.t.h.as<uint8_t>() + b.L.spans, L.NG * 8);
    memset(o->flags, 0, L.NG);
  }
}

// A scan from the slot's pinned twin into the caller's zke_sig_scan: statuses, the CSR over the record slots in use (the
// compaction: one memcpy per e-mail), the selector bytes.  ZKE_E_NOMEM when sigs or sel_blob is too small (*_need says how much).
int deliver_scan(zke_engine* e, const ScanBufs& b, zke_sig_scan* o) {
  const ScanLayout& S = b.L;
  const uint8_t* hp = b.t.h.as<uint8_t>();
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
  const uint8_t* hp = b.t.h.as<uint8_t>();
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

// An extraction from the slot's pinned twin into the caller's zke_body_out (host_stage.hip.h: body_measure, body_compact): the infos
// with body_off rewritten to the packed offsets, the bodies compacted.  The second places (bodies that outgrew their e-mail) are
// fetched only when one is in use.  ZKE_E_NOMEM when bytes is too small (bytes_need says how much).
int deliver_body(zke_engine* e, const BodyBufs& b, zke_body_out* o, hipStream_t s) {
  const BodyLayout& K = b.L;
  uint8_t* hp = b.t.h.as<uint8_t>();
  bool spilled = false;
  const int r = body_measure(K, hp, o, spilled);
  if (r == ZKE_E_DEVICE) return fail(e, r, "body extraction: an info points outside its e-mail's place");
  if (r) return fail(e, r, "body extraction: bytes is smaller than the decoded bodies (zke_body_out.bytes_need)");
  if (spilled) {
    HIPCHK(e, hipMemcpyAsync(hp + K.first_copy, b.t.d.as<uint8_t>() + K.first_copy, K.region, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  }
  body_compact(K, hp, o);
  return 0;
}

// The encodings from the slot's pinned twin into the caller's zke_encoded_out (both buffers were checked against the plan's exact
// sizes before the batch was staged): the infos as they are, the bytes in runs of encoded e-mails that follow each other — the place
// of an e-mail that was not encoded holds whatever the slot's buffer held, and the caller's bytes stay as they were there.  An info
// that points outside the blob is refused and nothing is read through it.
int deliver_encoded(zke_engine* e, const EncBufs& b, zke_encoded_out* o) {
  const EncLayout& K = b.L;
  const uint8_t* hp = b.t.h.as<uint8_t>();
  const zke_encoded_info* src = reinterpret_cast<const zke_encoded_info*>(hp);
  for (uint32_t i = 0; i < K.n; i++)
    if (src[i].off > K.blob || src[i].len > K.blob - src[i].off) return fail(e, ZKE_E_DEVICE, "output encoding: an info points outside the blob");
  if (K.n) memcpy(o->infos, src, (size_t)K.n * sizeof(zke_encoded_info));
  uint64_t r0 = 0, r1 = 0;
  auto flush = [&] { if (r1 > r0) memcpy(o->bytes + r0, hp + K.bytes + r0, (size_t)(r1 - r0)); };
  for (uint32_t i = 0; i < K.n; i++) {
    if (!src[i].len) continue;
    if (src[i].off != r1) { flush(); r0 = src[i].off; }
    r1 = src[i].off + src[i].len;
  }
  flush();
  return 0;
}

// The encodings of a device-planned batch (zke_extract_captures_encoded): the infos from the slot's pinned twin, the exact needs from
// the gather launch's header (the capture buffer's twin), then the bytes from HBM in runs of written e-mails that follow each other,
// as deliver_encoded copies them: a complete batch is ONE run from 0, of exactly its size; where an e-mail had no room (its place is
// kept, nothing of it was written) the run ends, and the caller's bytes stay as they were there.  ZKE_E_NOMEM when bytes is too small for the
// encodings (bytes_need says how much) or the strings did not fit their blob (the e-mails concerned have len 0): infos and needs
// are delivered all the same.  An info that points outside the device blob is refused and nothing is read through it.
int deliver_encoded_planned(zke_engine* e, const EncBufs& b, const CapBufs& cb, zke_encoded_out* o, hipStream_t s) {
  const EncLayout& K = b.L;
  const zke_encoded_info* src = reinterpret_cast<const zke_encoded_info*>(b.t.h.as<uint8_t>());
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(cb.t.h.as<uint8_t>() + cb.L.hdr);
  for (uint32_t i = 0; i < K.n; i++) {
    if (!src[i].len) continue;          // (its off is the planned place, which may lie beyond a blob that is too small)
    if (src[i].off > K.blob || src[i].len > K.blob - src[i].off) return fail(e, ZKE_E_DEVICE, "output encoding: an info points outside the blob");
  }
  if (K.n) memcpy(o->infos, src, (size_t)K.n * sizeof(zke_encoded_info));
  o->infos_need = K.n; o->bytes_need = (size_t)hdr[2];
  uint64_t r0 = 0, r1 = 0;
  bool copied = false;
  hipError_t he = hipSuccess;
  auto flush = [&] {
    if (r1 > r0 && he == hipSuccess) { he = hipMemcpyAsync(o->bytes + r0, b.t.d.as<uint8_t>() + K.bytes + r0, (size_t)(r1 - r0), hipMemcpyDeviceToHost, s); copied = true; }
  };
  for (uint32_t i = 0; i < K.n; i++) {
    if (!src[i].len) continue;
    if (src[i].off != r1) { flush(); r0 = src[i].off; }
    r1 = src[i].off + src[i].len;
  }
  flush();
  if (copied) {
    const hipError_t hs = hipStreamSynchronize(s);      // also behind a failed copy: none outlives the caller's buffer
    if (he != hipSuccess || hs != hipSuccess) return fail(e, ZKE_E_DEVICE, "output encoding: copy", he != hipSuccess ? he : hs);
  }
  if (hdr[2] > K.blob) return fail(e, ZKE_E_NOMEM, "output encoding: bytes is smaller than the encodings (zke_encoded_out.bytes_need)");
  if (hdr[1] > cb.L.blob_cap) return fail(e, ZKE_E_NOMEM, "output encoding: the capture strings did not fit cap_blob (zke_capture_out.cap_blob_need)");
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

// Pay what a slot owes for a batch whose last copy has arrived, from the slot's pinned buffers into the caller's.  The order: the
// records, the selection fold, the scan, the key records, the bodies, the captures, the origins, the encodings.  Needs no device where
// nothing is left in HBM (a body that did not spill, no capture strings).
// The shortfall rule: an output whose variable-size buffer is too small is ZKE_E_NOMEM to whoever waits — `cap_rc` (zke_batch_wait,
// the synchronous entries) — and nobody's business otherwise: a slot that retires a batch nobody waited for has nobody to tell, and
// zke_last_error stays what it was.  Everything of fixed size and every *_need is delivered either way; any other error ends the delivery.
int deliver_pending(zke_engine* e, Slot& w, const PendingDelivery& d, int* cap_rc) {
  if (d.records && d.n) memcpy(d.records, w.h_results.p, (size_t)d.n * sizeof(zke_result));
  if (!d.sel_off.empty()) fold_selection(w.h_results.as<zke_result>(), d.sel_off, d.sel_out, d.sel_chosen);
  const std::string keep = cap_rc ? std::string() : g_err;
  auto settled = [&](int r) {      // the shortfall rule
    if (r == ZKE_E_NOMEM) { if (cap_rc) *cap_rc = r; else g_err = keep; }
    return r == ZKE_E_NOMEM ? 0 : r;
  };
  int r = 0;
  if (d.scan && (r = settled(deliver_scan(e, w.sb, d.scan)))) return r;
  if (d.keyrec && (r = settled(deliver_keyrec(e, w.kb, d.keyrec)))) return r;
  if (d.body && (r = settled(deliver_body(e, w.bb, d.body, w.stream)))) return r;
  if (d.caps && (r = settled(deliver_captures(e, w.cb, d.caps, w.stream)))) return r;
  if (d.org) deliver_origins(w.cb, w.ob, d.org);
  if (d.enc && d.enc_planned) return settled(deliver_encoded_planned(e, w.eb, w.cb, d.enc, w.stream));
  if (d.enc && (r = deliver_encoded(e, w.eb, d.enc))) return r;
  return 0;
}

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

// A host batch, checked and measured for the staging image by host_batch(): packed (zke_batch) or gathered (zke_email_ref[n]).
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
  ImageLayout L{};
};
// The plan sections of a batch's image, one behind the other: a mixed batch's plan, a mixed extraction's tables, an encoding's jobs
// and external inputs (which start 64-byte aligned: a blob lies in them).
size_t enc_image_at(const HostBatch& d) {
  return align_up((d.mixed ? mixed_image(d.b.n, d.mixed->shape).total : 0) + (d.capmix ? d.capmix->image(d.b.n).total : 0), 64);
}
void layout_host_batch(HostBatch& d) {
  const size_t plans = d.enc ? enc_image_at(d) + d.enc->image().total
                             : (d.mixed ? mixed_image(d.b.n, d.mixed->shape).total : 0) + (d.capmix ? d.capmix->image(d.b.n).total : 0);
  d.L = image_layout(d.b.n, d.raw_total, d.dom_total, d.key_total, d.cap_words, d.cap_strs, d.cap_bytes, plans);
}
// Both shapes.  Capture tables: a cap_off whose last entry is 0 holds no string and is no table (cap_str_off, cap_blob unread).
int measure_host_batch(HostBatch& d, const char* who) {
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
  layout_host_batch(d);
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
// of lists: the capture tables are its; `capmix`: the mixed extraction whose regex stage `mixed` is.
int host_batch(HostBatch& d, const char* who, const zke_result* out, const zke_email_ref* refs, uint32_t n, const zke_regex_lists* lists,
               MixedReq* mixed = nullptr, CapMixedReq* capmix = nullptr) {
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
  return measure_host_batch(d, who);
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

// One host batch into slot w (caller holds its lock): the side outputs' buffers, then pack -> one H2D -> the launches (one stand-alone
// side launch, or the verify pipeline, behind the key-record prefix if the keys come as records) -> the D2H of every twin -> event, and
// the slot owes the delivery.
int submit_host(zke_engine* e, Slot& w, const HostBatch& d, zke_result* out, bool want_em, bool want_clean) {
  const uint32_t n = d.b.n;
  const ImageLayout& L = d.L;
  int rc = 0;
  if ((rc = retire_host(e, w))) return rc;           // the pinned buffers are about to be overwritten
  if ((rc = ensure_host_buffers(e, w, L.total, n))) return rc;      // (a no-op: submit_host_batch has grown every slot's staging)
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
  const MixedImage ML = d.mixed ? mixed_image(n, d.mixed->shape) : MixedImage{};
  if (d.mixed) {           // the plan of a mixed batch rides in the same image: the batch is still ONE copy
    const MixedPlan& P = d.mixed->plan;
    uint8_t* mp = hp + L.mixed;
    stage_copy(mp + ML.job_off, P.job_off.data(), P.job_off.size() * 4);
    stage_copy(mp + ML.email_cfg, P.email_cfg.data(), P.email_cfg.size() * 4);
    stage_copy(mp + ML.perm, P.perm.data(), P.perm.size() * 4);
    stage_copy(mp + ML.segs, P.segs.data(), P.segs.size() * sizeof(MixedSeg));
  }
  const CapMixedImage CL = d.capmix ? d.capmix->image(n) : CapMixedImage{};
  if (d.capmix) {          // a mixed extraction's columns and its part table, one more section behind the plan
    const CapMixedPlan& P = d.capmix->plan;
    uint8_t* cp = hp + L.mixed + ML.total;
    stage_copy(cp + CL.col_off, P.col_off.data(), P.col_off.size() * 4);
    stage_copy(cp + CL.cap_cfg, P.cap_cfg.data(), P.cap_cfg.size() * 4);
    stage_copy(cp + CL.cfgs, P.cfgs.data(), P.cfgs.size() * sizeof(CapMixedCfg));
    stage_copy(cp + CL.parts, d.capmix->part.data(), d.capmix->part.size() * sizeof(CapPartDev));
  }
  const EncImage EL = d.enc ? d.enc->image() : EncImage{};
  const size_t enc_at = d.enc ? L.mixed + enc_image_at(d) : 0;
  if (d.enc) {             // an encoding's jobs and its external-input table, the last of the plan sections
    const EncodePlan& P = d.enc->plan;
    if (d.enc->device_plan) { if (P.ext_strs) stage_copy(hp + enc_at + EL.jobs, d.enc->ext_off, ((size_t)n + 1) * 4); }
    else stage_copy(hp + enc_at + EL.jobs, P.jobs.data(), P.jobs.size() * sizeof(EncodeJob));
    if (P.ext_strs) stage_copy(hp + enc_at + EL.ext_str_off, d.enc->ext_str_off, ((size_t)P.ext_strs + 1) * 4);
    if (P.ext_bytes) stage_copy(hp + enc_at + EL.ext_blob, d.enc->ext_blob, P.ext_bytes);
  }
  hipStream_t s = w.stream;
  SlotUse use(e, w, s);
  if ((rc = use.acquire())) return rc;
  StageTimer tm(e, &w, s);
  tm.mark(MK_START);
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
  if (d.scan) rc = launch_scan(e, w.sb, dv, batch_clock(e), tm, s);
  else if (d.body) rc = launch_body(e, w.bb, dv, d.body->flags, tm, s);
  else if (d.keyrec && !d.sel) rc = launch_keyrec(e, w.kb, dv, d.keyrec->mode, tm, s);
  else {
    uint64_t key_hint = d.key_total;
    if (d.keyrec) {
      if ((rc = launch_keyrec_prefix(e, w.kb, dv, d.keyrec->mode, s))) return rc;
      // (run_device_pipeline reads "the keys average more than an RSA-2048 key's 270 bytes" from the total: a 2048-bit
      // SubjectPublicKeyInfo record is about 410 characters, a 3072-bit one 580)
      key_hint = d.key_total > (uint64_t)n * 480 ? (uint64_t)n * 273 : 0;
    }
    const uint8_t* mp = dp + L.mixed;
    const MixedLaunch ml{d.mixed ? &d.mixed->plan : nullptr, reinterpret_cast<const uint32_t*>(mp + ML.job_off), reinterpret_cast<const uint32_t*>(mp + ML.email_cfg),
                         reinterpret_cast<const uint32_t*>(mp + ML.perm), reinterpret_cast<const MixedSeg*>(mp + ML.segs)};
    const uint8_t* cp = mp + ML.total;
    const CapMixedLaunch cl{d.capmix ? d.capmix->plan.shape.J : 0u, d.capmix ? d.capmix->plan.shape.Gt : 0u, d.capmix && d.capmix->needs_work,
                            d.capmix && d.capmix->origin_launch(),
                            CapMixedTables{ml.job_off, reinterpret_cast<const uint32_t*>(cp + CL.col_off), reinterpret_cast<const uint32_t*>(cp + CL.cap_cfg),
                                           reinterpret_cast<const CapMixedCfg*>(cp + CL.cfgs), reinterpret_cast<const CapPartDev*>(cp + CL.parts)}};
    const bool planned = d.enc && d.enc->device_plan;
    if (planned) {         // the gather launch of this extraction also plans the encoding: where it reads the external inputs, where the jobs go
      d.cap->lossy_ext_off = d.enc->plan.ext_strs ? reinterpret_cast<const uint32_t*>(dp + enc_at + EL.jobs) : nullptr;
      d.cap->lossy_ext_str_off = reinterpret_cast<const uint32_t*>(dp + enc_at + EL.ext_str_off);
      d.cap->lossy_jobs = reinterpret_cast<EncodeJob*>(w.eb.t.d.as<uint8_t>() + w.eb.jobs_at);
      d.cap->lossy_bytes_cap = d.enc->bytes_cap;
    }
    if ((rc = run_device_pipeline(e, w, &dv, d.raw_total, key_hint, w.d_results.as<zke_result>(), s, want_em, batch_clock(e), want_clean, d.cap,
                                  d.mixed ? &ml : nullptr, d.capmix ? &cl : nullptr))) return rc;
    if (d.enc) {           // the encodings of the records just written and their digests, two more launches on the same stream
      EncodeArgs ea{};
      ea.records = w.d_results.as<zke_result>();
      ea.jobs = planned ? d.cap->lossy_jobs : reinterpret_cast<const EncodeJob*>(dp + enc_at + EL.jobs);
      ea.ext_str_off = reinterpret_cast<const uint32_t*>(dp + enc_at + EL.ext_str_off); ea.ext_blob = dp + enc_at + EL.ext_blob;
      ea.match_str_off = dv.cap_str_off; ea.match_blob = dv.cap_blob;
      if (planned) {       // the matches are the tables the gather launch has just written in the slot's capture buffer
        ea.match_str_off = reinterpret_cast<const uint32_t*>(w.cb.t.d.as<uint8_t>() + w.cb.L.cap_str_off);
        ea.match_blob = w.cb.t.d.as<uint8_t>() + w.cb.L.blob;
      }
      if ((rc = launch_encode(e, w.eb, ea, s, planned))) return rc;
    }
    HIPCHK(e, hipMemcpyAsync(w.h_results.p, w.d_results.p, (size_t)n * sizeof(zke_result), hipMemcpyDeviceToHost, s));
    if (d.enc) HIPCHK(e, w.eb.t.fetch(planned ? w.eb.L.bytes : w.eb.L.prefix, s));
    if (d.keyrec) HIPCHK(e, w.kb.t.fetch(w.kb.L.total, s));
  }
  if (rc) return rc;
  if (d.cap || d.capmix) HIPCHK(e, w.cb.t.fetch(w.cb.L.fixed_end, s));
  if (((d.cap && d.cap->org) || (d.capmix && d.capmix->org)) && w.ob.launched) HIPCHK(e, w.ob.t.fetch(w.ob.L.total, s));
  tm.mark(MK_D2H);
  HIPCHK(e, hipEventRecord(w.host_done, s));
  w.host_gen++;
  w.owed = pending_delivery(d, out);
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
// The request of a mixed batch from the caller's zke_regex_mixed: the checks that need no registry, the configs' part counts, the shape.
int mixed_request(const char* who, const zke_regex_mixed* mixed, uint32_t n, MixedReq& q) {
  if (mixed->n_configs > ZKE_MIXED_MAX_CONFIGS) return arg_error(who, "more than ZKE_MIXED_MAX_CONFIGS configs");
  if ((mixed->n_configs && !mixed->configs) || (n && !mixed->config_of)) return arg_error(who, "null pointer");
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
  if (int r = host_batch(d, who, out, emails, n, in->lists, in->mixed ? &mq : nullptr)) return r;
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

// The two launches alone over the caller's records and tables (host pointers), beside zke_sha256_batch: one staged input
// {records | jobs | the two tables}, the slot's encoding buffer — the one the entry above uses —, one copy back.  Synchronous.
int zke_encode_outputs(zke_engine* e, const zke_result* records, uint32_t n, const uint32_t* kinds, const uint32_t* ext_off,
                       const uint32_t* ext_str_off, const uint8_t* ext_blob, const uint32_t* match_off, const uint32_t* match_str_off,
                       const uint8_t* match_blob, zke_encoded_out* enc) {
  static const char who[] = "zke_encode_outputs";
  if (!e) return ZKE_E_ARG;
  if (!enc || (n && (!records || !kinds))) return arg_error(who, "null pointer");
  EncodeTables t;
  t.ext_off = ext_off; t.ext_str_off = ext_str_off; t.ext_blob = ext_blob;
  t.match_off = match_off; t.match_str_off = match_str_off; t.match_blob = match_blob;
  EncodePlan P;
  if (const char* why = encode_plan_build(n, kinds, t, P)) return arg_error(who, why);
  if (int r = check_encoded_out(enc, n, P.total, who)) return r;
  if (n == 0) return 0;
  size_t o = 0;
  auto put = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 64); return at; };
  const size_t at_rec = put((size_t)n * sizeof(zke_result)), at_jobs = put((size_t)n * sizeof(EncodeJob));
  const size_t at_eso = put(P.ext_strs ? ((size_t)P.ext_strs + 1) * 4 : 0), at_eb = put(P.ext_bytes);
  const size_t at_mso = put(P.match_strs ? ((size_t)P.match_strs + 1) * 4 : 0), at_mb = put(P.match_bytes);
  std::vector<uint8_t> img(o);
  memcpy(img.data() + at_rec, records, (size_t)n * sizeof(zke_result));
  memcpy(img.data() + at_jobs, P.jobs.data(), (size_t)n * sizeof(EncodeJob));
  if (P.ext_strs) memcpy(img.data() + at_eso, ext_str_off, ((size_t)P.ext_strs + 1) * 4);
  if (P.ext_bytes) memcpy(img.data() + at_eb, ext_blob, P.ext_bytes);
  if (P.match_strs) memcpy(img.data() + at_mso, match_str_off, ((size_t)P.match_strs + 1) * 4);
  if (P.match_bytes) memcpy(img.data() + at_mb, match_blob, P.match_bytes);
  std::shared_lock<std::shared_mutex> sh(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  uint32_t slot;
  Slot& w = next_slot(e, slot);
  std::lock_guard<std::mutex> g(w.mu);
  int r = 0;
  if ((r = retire_host(e, w))) return r;             // the buffer's pinned twin may hold encodings nobody has waited for yet
  if ((r = ensure_encode_buffers(e, w.eb, n, P.total, img.size()))) return r;
  hipStream_t s = w.stream;
  SlotUse use(e, w, s);
  if ((r = use.acquire())) return r;
  auto enqueue = [&]() -> int {
    HIPCHK(e, hipMemcpyAsync(w.eb.in.p, img.data(), img.size(), hipMemcpyHostToDevice, s));
    const uint8_t* ip = w.eb.in.as<uint8_t>();
    EncodeArgs ea{};
    ea.records = reinterpret_cast<const zke_result*>(ip + at_rec);
    ea.jobs = reinterpret_cast<const EncodeJob*>(ip + at_jobs);
    ea.ext_str_off = reinterpret_cast<const uint32_t*>(ip + at_eso); ea.ext_blob = ip + at_eb;
    ea.match_str_off = reinterpret_cast<const uint32_t*>(ip + at_mso); ea.match_blob = ip + at_mb;
    if (int lr = launch_encode(e, w.eb, ea, s)) return lr;
    HIPCHK(e, w.eb.t.fetch(w.eb.L.prefix, s));
    return use.release();
  };
  r = enqueue();
  const hipError_t hs = hipStreamSynchronize(s);      // also behind a failed enqueue: no copy outlives `img`
  if (r) return r;
  if (hs != hipSuccess) return fail(e, ZKE_E_DEVICE, "zke_encode_outputs: sync", hs);
  return deliver_encoded(e, w.eb, enc);
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

// zke_extract_captures_async and its mapped form (`mapped`: org is wanted, and checked behind caps)
int extract_captures_submit(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_part* header_parts,
                            uint32_t n_header_parts, const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out,
                            zke_capture_out* caps, bool mapped, zke_capture_origin* org, uint64_t* ticket, const char* who) {
  if (!e) return ZKE_E_ARG;
  if (!ticket || !caps || (mapped && !org) || (n_header_parts && !header_parts) || (n_body_parts && !body_parts)) return arg_error(who, "null pointer");
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
  const uint32_t P = n_header_parts + n_body_parts;
  if (P == 0 || P > ZKE_CAP_MAX_PARTS || n_header_parts > ZKE_CAP_MAX_PARTS) return arg_error(who, "1 .. ZKE_CAP_MAX_PARTS parts");
  CaptureReq q;
  q.P = P; q.n_header_parts = n_header_parts; q.out = caps; q.lossy = true;
  q.dfa_ids.resize(P);
  for (uint32_t p = 0; p < P; p++) {
    const zke_capture_part& cp = p < n_header_parts ? header_parts[p] : body_parts[p - n_header_parts];
    q.dfa_ids[p] = cp.dfa_id;
    if (int r = capture_part_shape(q, p, cp.prog_id, cp.groups, cp.n_groups, who)) return r;
  }
  // a repaired string is at most three times its span: what n * G of those could not address in 32 bits is refused
  const uint64_t str_worst = 3ull * ZKE_CAP_MAX_SPAN, blob_worst = (uint64_t)n * q.G * str_worst;
  if (blob_worst > 0xFFFFFFFFull) return arg_error(who, "n x groups beyond what 32-bit string offsets address (n * G * 3 * ZKE_CAP_MAX_SPAN must stay below 4 GiB): split the batch");
  if (caps) if (int r = check_capture_out(caps, n, P, q.G, who)) return r;
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
  if (int r = host_batch(d, who, out, emails, n, &lists)) return r;
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
  if (mixed->n_configs > ZKE_MIXED_MAX_CONFIGS) return arg_error(who, "more than ZKE_MIXED_MAX_CONFIGS configs");
  if ((mixed->n_configs && !mixed->configs) || (n && !mixed->config_of)) return arg_error(who, "null pointer");
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

// ---- capture extraction over haystacks of the caller's (registry.hip.h), with the checks and the delivery of the entries above
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
  Scoped<CapBufs> tmp;
  Scoped<DevBuf> dhay, doff, dparts;
  std::vector<uint8_t> fixed;
  int r = 0;
  hipError_t he = hipSuccess;
  tmp.L = cap_layout(n, 1, q.G, caps->cap_blob_cap);
  const CapLayout& L = tmp.L;
  hipStream_t s = e->stream;
  if ((r = dhay.ensure((size_t)total + 64)) || (r = doff.ensure((size_t)(n + 1) * 8)) || (r = dparts.ensure((size_t)n * sizeof(PartRes))) ||
      (r = ensure_capture_buffers(e, tmp, L, q.needs_work)))
    return fail(e, r, "zke_capture_batch: allocation");
  std::vector<uint64_t> rel(n + 1);
  for (uint32_t i = 0; i <= n; i++) rel[i] = hay_off[i] - base0;
  if (total) he = hipMemcpyAsync(dhay.p, hay_blob + base0, (size_t)total, hipMemcpyHostToDevice, s);
  if (he == hipSuccess) he = hipMemsetAsync(dhay.as<uint8_t>() + total, 0, 64, s);         // the DFA walk loads 16 bytes at a time
  if (he == hipSuccess) he = hipMemcpyAsync(doff.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s);
  if (he != hipSuccess) { (void)hipStreamSynchronize(s); return fail(e, ZKE_E_DEVICE, "zke_capture_batch: copy", he); }
  CapFindArgs fa{};
  fa.d.re = pi.dev; fa.d.P = 1; fa.d.out = dparts.as<PartRes>(); fa.d.idle = 0xFFFFFFFFu; fa.d.decode_detail = pi.detail;
  fa.hay_blob = dhay.as<uint8_t>(); fa.hay_off = doff.as<uint64_t>(); fa.n = n;
  hipLaunchKernelGGL(capture_find_kernel, dim3((n + 255) / 256), dim3(256), 1024, s, fa);
  r = launch_capture(e, tmp, q, n, true, DfaArgs{}, fa.hay_blob, fa.hay_off, dparts.as<PartRes>(), nullptr, s);
  std::vector<PartRes> prs(n);
  if (!r) {
    he = tmp.t.fetch(L.fixed_end, s);
    if (he == hipSuccess) he = hipMemcpyAsync(prs.data(), dparts.p, (size_t)n * sizeof(PartRes), hipMemcpyDeviceToHost, s);
  }
  const hipError_t hs = hipStreamSynchronize(s);
  if (r) return r;
  if (he != hipSuccess || hs != hipSuccess) return fail(e, ZKE_E_DEVICE, "zke_capture_batch", he != hipSuccess ? he : hs);
  const uint32_t* codes = reinterpret_cast<const uint32_t*>(tmp.t.h.as<uint8_t>() + L.codes);
  for (uint32_t i = 0; i < n; i++) {
    const PartRes& pr = prs[i];
    const bool undecodable = pr.code == PART_DECODE_FAIL;
    matches[4 * i] = undecodable ? pr.count : (pr.code ? pr.code : codes[i]);
    matches[4 * i + 1] = undecodable ? 0 : pr.count; matches[4 * i + 2] = pr.start; matches[4 * i + 3] = pr.end;
  }
  return deliver_captures(e, tmp, caps, s);
}

// ---- remove_quoted_printable_soft_breaks with its index map over plain bodies (include/zkemail_amd.h; kernel: qpmap.hip.h).  One
// slot, its stream and its QpBufs (grow only); the caller's buffers are read and written by the copies themselves.
int zke_qp_clean_batch(zke_engine* e, const uint8_t* body_blob, const uint64_t* body_off, uint32_t n,
                       uint8_t* cleaned, uint32_t* index_map, uint32_t* clean_len) {
  static const char who[] = "zke_qp_clean_batch";
  if (!e) return ZKE_E_ARG;
  if (!cleaned && !index_map && !clean_len) return arg_error(who, "all three outputs are null");
  if (n == 0) return 0;
  if (!body_off) return arg_error(who, "null pointer");
  if (!rising(body_off, n)) return arg_error(who, "offset array is not non-decreasing");
  for (uint32_t i = 0; i < n; i++) if (body_off[i + 1] - body_off[i] >= 0xFFFFFFFFull) return arg_error(who, "body of 2^32 - 1 bytes or more");
  const uint64_t base0 = body_off[0], total = body_off[n] - base0;
  if (total && !body_blob) return arg_error(who, "null pointer");
  std::shared_lock<std::shared_mutex> sh(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  uint32_t slot;
  Slot& w = next_slot(e, slot);
  std::lock_guard<std::mutex> g(w.mu);
  QpBufs& b = w.qb;
  int r = 0;
  if ((r = b.in.ensure((size_t)total + 16)) || (r = b.off.ensure((size_t)(n + 1) * 8)) || (cleaned && (r = b.clean.ensure((size_t)total + 16))) ||
      (index_map && (r = b.map.ensure(((size_t)total + 4) * 4))) || (clean_len && (r = b.len.ensure((size_t)n * 4))))
    return fail(e, r, "zke_qp_clean_batch: allocation");
  hipStream_t s = w.stream;
  SlotUse use(e, w, s);
  if ((r = use.acquire())) return r;
  auto enqueue = [&]() -> int {
    if (total) HIPCHK(e, hipMemcpyAsync(b.in.p, body_blob + base0, (size_t)total, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(b.off.p, body_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));      // (as given: the kernel subtracts off[0])
    const QpIndexArgs qa{n, b.in.as<uint8_t>(), b.off.as<uint64_t>(), cleaned ? b.clean.as<uint8_t>() : nullptr,
                         index_map ? b.map.as<uint32_t>() : nullptr, clean_len ? b.len.as<uint32_t>() : nullptr};
    hipLaunchKernelGGL(qp_index_kernel, dim3(std::min<uint32_t>(n, 1u << 16)), dim3(64), 0, s, qa);
    HIPCHK(e, hipGetLastError());
    if (cleaned && total) HIPCHK(e, hipMemcpyAsync(cleaned, b.clean.p, (size_t)total, hipMemcpyDeviceToHost, s));
    if (index_map && total) HIPCHK(e, hipMemcpyAsync(index_map, b.map.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    if (clean_len) HIPCHK(e, hipMemcpyAsync(clean_len, b.len.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    return use.release();
  };
  r = enqueue();
  const hipError_t hs = hipStreamSynchronize(s);      // also behind a failed enqueue: no copy outlives the caller's buffers
  if (r) return r;
  if (hs != hipSuccess) return fail(e, ZKE_E_DEVICE, "zke_qp_clean_batch: sync", hs);
  return 0;
}

// ---- String::from_utf8_lossy over plain strings (include/zkemail_amd.h; kernels: utf8_lossy.hip.h).  One slot, its stream and its
// Utf8Bufs (grow only).  The repaired blob on the device holds min(out_blob_cap, 3 * the input) bytes — no string grows further — and
// the write launch leaves out what would end beyond it; the offsets come back first, the bytes once the need is known to fit.
int zke_utf8_lossy_batch(zke_engine* e, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t* out_off, uint8_t* out_blob,
                         size_t out_blob_cap, size_t* out_blob_need, uint8_t* flags) {
  static const char who[] = "zke_utf8_lossy_batch";
  if (!e) return ZKE_E_ARG;
  if (!out_off || !out_blob_need || (n && (!off || !flags)) || (out_blob_cap && !out_blob)) return arg_error(who, "null pointer");
  if (n == 0) { out_off[0] = 0; *out_blob_need = 0; return 0; }
  if (!rising(off, n)) return arg_error(who, "offset array is not non-decreasing");
  const uint64_t base0 = off[0], total = off[n] - base0;
  if (total > ZKE_UTF8_LOSSY_MAX_BYTES) return arg_error(who, "more than ZKE_UTF8_LOSSY_MAX_BYTES bytes of strings (the repaired offsets are 32-bit)");
  if (total && !blob) return arg_error(who, "null pointer");
  std::shared_lock<std::shared_mutex> sh(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  uint32_t slot;
  Slot& w = next_slot(e, slot);
  std::lock_guard<std::mutex> g(w.mu);
  Utf8Bufs& b = w.ub;
  const uint64_t dev_cap = std::min<uint64_t>(out_blob_cap, 3 * total);
  int r = 0;
  if ((r = b.in.ensure((size_t)total + 16)) || (r = b.off.ensure((size_t)(n + 1) * 8)) || (r = b.out_off.ensure((size_t)(n + 1) * 4)) ||
      (r = b.out.ensure((size_t)dev_cap + 16)) || (r = b.flags.ensure(n)))
    return fail(e, r, "zke_utf8_lossy_batch: allocation");
  hipStream_t s = w.stream;
  SlotUse use(e, w, s);
  if ((r = use.acquire())) return r;
  auto enqueue = [&]() -> int {
    if (total) HIPCHK(e, hipMemcpyAsync(b.in.p, blob + base0, (size_t)total, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(b.off.p, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));      // (as given: the kernels subtract off[0])
    const Utf8LossyArgs ua{n, b.in.as<uint8_t>(), b.off.as<uint64_t>(), b.out_off.as<uint32_t>(), b.out.as<uint8_t>(), dev_cap, b.flags.as<uint8_t>()};
    const dim3 grid(std::min<uint32_t>(n, 1u << 16));
    hipLaunchKernelGGL(utf8_lossy_len_kernel, grid, dim3(64), 0, s, ua);
    hipLaunchKernelGGL(utf8_lossy_scan_kernel, dim3(1), dim3(1024), 0, s, ua);
    hipLaunchKernelGGL(utf8_lossy_write_kernel, grid, dim3(64), 0, s, ua);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(out_off, b.out_off.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(flags, b.flags.p, n, hipMemcpyDeviceToHost, s));
    return use.release();
  };
  r = enqueue();
  hipError_t hs = hipStreamSynchronize(s);      // also behind a failed enqueue: no copy outlives the caller's buffers
  if (r) return r;
  if (hs != hipSuccess) return fail(e, ZKE_E_DEVICE, "zke_utf8_lossy_batch: sync", hs);
  const size_t need = out_off[n];
  *out_blob_need = need;
  if (need > out_blob_cap) return fail(e, ZKE_E_NOMEM, "zke_utf8_lossy_batch: out_blob is smaller than the repaired strings (*out_blob_need)");
  if (need) {
    HIPCHK(e, hipMemcpyAsync(out_blob, b.out.p, need, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  }
  return 0;
}

}  // extern "C"
