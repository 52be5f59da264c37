// host_blocks.hip.h — the synchronous building blocks: launches of the pipeline alone over the caller's own arrays (zke_encode_outputs,
// zke_capture_batch, zke_qp_clean_batch, zke_utf8_lossy_batch).  None touches a HostBatch; they share the host entries' checks and
// deliveries (host_entry.hip.h, host_deliver.hip.h), behind which engine.hip includes this file.
#pragma once

namespace {

// The skeleton of a block that runs on the next slot's stream: the slot and its lock, `ensure(w)` — the slot's buffers for this call —,
// the slot's use of its stream around `enqueue(w, s)`, the wait for the stream, then `finish(w, s)`, still under the slot's lock.  The
// stream is synchronised also behind a failed enqueue: no copy outlives the caller's buffers.  sync_error: the text of a failed wait.
template <class Ensure, class Enqueue, class Finish>
int run_block_on_slot(zke_engine* e, const char* sync_error, Ensure ensure, Enqueue enqueue, Finish finish) {
  std::shared_lock<std::shared_mutex> sh(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  uint32_t slot;
  Slot& w = next_slot(e, slot);
  std::lock_guard<std::mutex> g(w.mu);
  int r = 0;
  if ((r = ensure(w))) return r;
  hipStream_t s = w.stream;
  SlotUse use(e, w, s);
  if ((r = use.acquire())) return r;
  if (!(r = enqueue(w, s))) r = use.release();
  const hipError_t hs = hipStreamSynchronize(s);
  if (r) return r;
  if (hs != hipSuccess) return fail(e, ZKE_E_DEVICE, sync_error, hs);
  return finish(w, s);
}

}  // namespace

extern "C" {

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
  auto ensure = [&](Slot& w) -> int {
    if (int r = retire_host(e, w)) return r;         // the buffer's pinned twin may hold encodings nobody has waited for yet
    return ensure_encode_buffers(e, w.eb, n, P.total, img.size());
  };
  auto enqueue = [&](Slot& w, hipStream_t s) -> int {
    HIPCHK(e, hipMemcpyAsync(w.eb.in.p, img.data(), img.size(), hipMemcpyHostToDevice, s));
    const uint8_t* ip = w.eb.in.as<uint8_t>();
    EncodeArgs ea{};
    ea.records = reinterpret_cast<const zke_result*>(ip + at_rec);
    ea.jobs = reinterpret_cast<const EncodeJob*>(ip + at_jobs);
    ea.ext_str_off = reinterpret_cast<const uint32_t*>(ip + at_eso); ea.ext_blob = ip + at_eb;
    ea.match_str_off = reinterpret_cast<const uint32_t*>(ip + at_mso); ea.match_blob = ip + at_mb;
    if (int lr = launch_encode(e, w.eb, ea, s)) return lr;
    HIPCHK(e, w.eb.t.fetch(w.eb.L.prefix, s));
    return 0;
  };
  return run_block_on_slot(e, "zke_encode_outputs: sync", ensure, enqueue, [&](Slot& w, hipStream_t) { return deliver_encoded(e, w.eb, enc); });
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
  const PartInfo pi = [&] { std::shared_lock<std::shared_mutex> rl(e->reg_mu); return part_info(e, dfa_id); }();
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
  auto ensure = [&](Slot& w) -> int {
    QpBufs& b = w.qb;
    int r = 0;
    if ((r = b.in.ensure((size_t)total + 16)) || (r = b.off.ensure((size_t)(n + 1) * 8)) || (cleaned && (r = b.clean.ensure((size_t)total + 16))) ||
        (index_map && (r = b.map.ensure(((size_t)total + 4) * 4))) || (clean_len && (r = b.len.ensure((size_t)n * 4))))
      return fail(e, r, "zke_qp_clean_batch: allocation");
    return 0;
  };
  auto enqueue = [&](Slot& w, hipStream_t s) -> int {
    QpBufs& b = w.qb;
    if (total) HIPCHK(e, hipMemcpyAsync(b.in.p, body_blob + base0, (size_t)total, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(b.off.p, body_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));      // (as given: the kernel subtracts off[0])
    const QpIndexArgs qa{n, b.in.as<uint8_t>(), b.off.as<uint64_t>(), cleaned ? b.clean.as<uint8_t>() : nullptr,
                         index_map ? b.map.as<uint32_t>() : nullptr, clean_len ? b.len.as<uint32_t>() : nullptr};
    hipLaunchKernelGGL(qp_index_kernel, dim3(std::min<uint32_t>(n, 1u << 16)), dim3(64), 0, s, qa);
    HIPCHK(e, hipGetLastError());
    if (cleaned && total) HIPCHK(e, hipMemcpyAsync(cleaned, b.clean.p, (size_t)total, hipMemcpyDeviceToHost, s));
    if (index_map && total) HIPCHK(e, hipMemcpyAsync(index_map, b.map.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    if (clean_len) HIPCHK(e, hipMemcpyAsync(clean_len, b.len.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    return 0;
  };
  return run_block_on_slot(e, "zke_qp_clean_batch: sync", ensure, enqueue, [](Slot&, hipStream_t) { return 0; });
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
  const uint64_t dev_cap = std::min<uint64_t>(out_blob_cap, 3 * total);
  auto ensure = [&](Slot& w) -> int {
    Utf8Bufs& b = w.ub;
    int r = 0;
    if ((r = b.in.ensure((size_t)total + 16)) || (r = b.off.ensure((size_t)(n + 1) * 8)) || (r = b.out_off.ensure((size_t)(n + 1) * 4)) ||
        (r = b.out.ensure((size_t)dev_cap + 16)) || (r = b.flags.ensure(n)))
      return fail(e, r, "zke_utf8_lossy_batch: allocation");
    return 0;
  };
  auto enqueue = [&](Slot& w, hipStream_t s) -> int {
    Utf8Bufs& b = w.ub;
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
    return 0;
  };
  return run_block_on_slot(e, "zke_utf8_lossy_batch: sync", ensure, enqueue, [&](Slot& w, hipStream_t s) -> int {
    const size_t need = out_off[n];
    *out_blob_need = need;
    if (need > out_blob_cap) return fail(e, ZKE_E_NOMEM, "zke_utf8_lossy_batch: out_blob is smaller than the repaired strings (*out_blob_need)");
    if (need) {
      HIPCHK(e, hipMemcpyAsync(out_blob, w.ub.out.p, need, hipMemcpyDeviceToHost, s));
      HIPCHK(e, hipStreamSynchronize(s));
    }
    return 0;
  });
}

}  // extern "C"
