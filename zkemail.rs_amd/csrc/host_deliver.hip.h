// host_deliver.hip.h — what a slot hands the caller of a finished host batch: every side output from the slot's pinned twin into the
// caller's struct (deliver_*), a key selection's fold, and deliver_pending, which pays a whole PendingDelivery (host_stage.hip.h) in
// its one order under the shortfall rule.  Host code that needs no device where nothing is left in HBM: tests/cpp/host_fuzz.cpp,
// keyrec_fuzz.cpp and body_fuzz.cpp drive it on the CPU.  Included by engine.hip behind pipeline.hip.h, in front of host_entry.hip.h.
#pragma once

namespace {

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

// The runs of encoded e-mails that follow each other in the blob, in order: copy(first byte, bytes) per run.  An e-mail of len 0 was
// not encoded and ends no run by itself; the first encoding that does not start where the last one ended does.
template <class CopyRun> void each_encoded_run(const zke_encoded_info* src, uint32_t n, CopyRun copy) {
  uint64_t r0 = 0, r1 = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!src[i].len) continue;
    if (src[i].off != r1) { if (r1 > r0) copy(r0, (size_t)(r1 - r0)); r0 = src[i].off; }
    r1 = src[i].off + src[i].len;
  }
  if (r1 > r0) copy(r0, (size_t)(r1 - r0));
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
  each_encoded_run(src, K.n, [&](uint64_t r0, size_t bytes) { memcpy(o->bytes + r0, hp + K.bytes + r0, bytes); });
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
  bool copied = false;
  hipError_t he = hipSuccess;
  each_encoded_run(src, K.n, [&](uint64_t r0, size_t bytes) {
    if (he == hipSuccess) { he = hipMemcpyAsync(o->bytes + r0, b.t.d.as<uint8_t>() + K.bytes + r0, bytes, hipMemcpyDeviceToHost, s); copied = true; }
  });
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

}  // namespace
