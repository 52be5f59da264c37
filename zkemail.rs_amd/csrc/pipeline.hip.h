// pipeline.hip.h — the device pipeline of one batch: workspace sizing, the kernel sequence of verify_email /
// verify_email_with_regex (core/src/circuits.rs:9-68), the capture launches behind it and the side launches that run in its place, timing marks, a slot's acquire / release,
// the entry for device-resident batches (zke_verify_batch_device).  Included by engine.hip (single translation unit).
#pragma once

namespace {

struct StageTimer {
  Slot* w; hipStream_t s; bool on;
  StageTimer(zke_engine* e_, Slot* w_, hipStream_t s_) : w(w_), s(s_), on(e_->timing.load()) {}
  void mark(int k) { if (on && hipEventRecord(w->ev[k], s) == hipSuccess) w->marks |= 1u << k; }
};

// Length-bucket counters start a batch at zero (the verdict launch of the slot's previous batch clears them): a fresh
// allocation is cleared here — on `s`, the stream the batch that reads them is launched on.  Not with hipMemset: on device memory
// that is a fill on the null stream which the call does not wait for, and the slots' streams are non-blocking ones that the null
// stream does not order either, so the first kernel of the batch could meet the counters as the allocator left them.
int ensure_zeroed(DevBuf& b, size_t need, hipStream_t s) {
  const void* old = b.p;
  if (int r = b.ensure(need)) return r;
  if (b.p != old && hipMemsetAsync(b.p, 0, b.cap, s) != hipSuccess) return ZKE_E_DEVICE;
  return 0;
}

// Workspace of one slot for batches of up to n e-mails / raw_total raw bytes (P regex parts; with_regex: the buffers of
// the canonicalize_signed_email pass too).  Grows only: in steady state — or after zke_engine_reserve — this allocates nothing.
// s: the stream the slot's next batch runs on; counters allocated here are cleared on it (ensure_zeroed).
int ensure_workspace(zke_engine* e, Slot& w, uint32_t n, uint64_t raw_total, bool with_regex, uint32_t P, bool want_em, hipStream_t s) {
  const uint32_t n_pad = (n + 63) & ~63u;
  int r = 0;
  const size_t scratch_bytes = 2 * (size_t)raw_total + (size_t)(n + 1) * SCR_PER_EMAIL + 256;
  if ((r = w.meta.ensure((size_t)n * sizeof(EmailMeta))) || (r = w.rsa_jobs.ensure((size_t)n * sizeof(RsaJob))) ||
      (r = w.sha_jobs.ensure((size_t)4 * n_pad * sizeof(ShaJob))) || (r = w.rsa_ok.ensure((size_t)n * 4)) ||
      (r = ensure_zeroed(w.sha_order, (size_t)2 * (SHA_ORDER_KIND_WORDS + n_pad) * 4, s)) ||
      (r = w.scratch_off.ensure((size_t)(n + 1) * 16)) || (r = w.scratch.ensure(scratch_bytes)))
    return fail(e, r, "workspace allocation");
  if (!w.pending.p) {       // counters: [0] e-mails pending another signature round, [2] length of the wave-routine job list (rsa_ok)
    if ((r = w.pending.ensure(64))) return fail(e, r, "workspace allocation");
    HIPCHK(e, hipMemsetAsync(w.pending.p, 0, 64, s));
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

// The DFA pair `id` as the registry holds it, copied out (the caller holds reg_mu; the entry itself stays put until the engine is idle).
PartInfo part_info(const zke_engine* e, uint32_t id) {
  PartInfo pi{};
  const RegisteredDfa* rd = id < e->dfas.size() ? e->dfas[id] : nullptr;
  if (rd) {
    pi.detail = rd->detail; pi.lds_bytes = rd->lds_bytes; pi.idle = rd->idle;
    pi.dev = rd->valid ? rd->dev.as<RegexDev>() : nullptr;
  }
  return pi;
}

int arg_error(const char* who, const char* what);      // (these three: host_entry.hip.h, behind this file)
int check_batch_pointers(const zke_batch* in, const void* out, bool host, const char* who);
int ensure_host_buffers(zke_engine* e, Slot& w, size_t image_bytes, uint32_t n);

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
  zke_capture_origin* org = nullptr;     // zke_extract_captures_mapped: the spans' origins before the QP filter are wanted too
  bool origin_launch() const { return org && G > gbase[n_header_parts]; }      // some body part asks for a group
  // zke_extract_captures_encoded: the gather launch is capture_gather_lossy_kernel (capture_lossy.hip.h) — repaired strings and the
  // encode plan.  `out` may then be null (nobody wants the tables); lossy_blob_cap is the device blob's capacity.
  bool lossy = false;
  size_t lossy_blob_cap = 0;
  size_t dev_blob_cap() const { return lossy ? lossy_blob_cap : out->cap_blob_cap; }
};
// Where the lossy gather launch of a request finds things in the slot (device pointers): the external inputs it reads from the staged
// image (ext_off: nullptr without external inputs), where the jobs it plans go, the capacity of the encodings behind them.
struct LossyLaunch {
  const uint32_t* ext_off; const uint32_t* ext_str_off;
  EncodeJob* jobs;
  uint64_t bytes_cap;
};
constexpr uint32_t CAP_WORK_WAVES = 256;      // waves of a capture launch whose rows live in the slot's workspace (one slice each)

// A side output's buffers, grow only (the first batch of a shape allocates, a later one of the same shape does not): the twin, then
// the extra device buffer where one is wanted.
int ensure_side_buffers(zke_engine* e, TwinBuf& t, size_t device_bytes, size_t pinned_bytes, DevBuf* extra, size_t extra_bytes, const char* what) {
  int r = 0;
  if ((r = t.ensure(device_bytes, pinned_bytes)) || (extra && (r = extra->ensure(extra_bytes)))) return fail(e, r, what);
  return 0;
}
// (b.L is the caller's to set: zke_engine_reserve grows a slot's capture buffers without touching the layout of a pending extraction)
int ensure_capture_buffers(zke_engine* e, CapBufs& b, const CapLayout& L, bool work) {
  return ensure_side_buffers(e, b.t, L.total, L.fixed_end, work ? &b.work : nullptr, (size_t)CAP_WORK_WAVES * CAP_WORK_WORDS * 8, "capture workspace allocation");
}

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
// One part against the registry (the caller holds reg_mu): its code and program; returns whether its rows need the workspace.
bool capture_resolve_part(const zke_engine* e, CapPartDev& d, uint32_t id) {
  const RegisteredCapture* rc = id < e->captures.size() ? e->captures[id] : nullptr;
  d.code = rc ? rc->detail : (uint32_t)ZKE_D_U_CAPTURE_PROGRAM;
  d.prog = CapProgDev{};
  if (rc && !rc->detail) { d.prog = rc->dev; return d.prog.words64 > CAP_LDS_WORDS; }
  return false;
}
void capture_resolve(zke_engine* e, CaptureReq& q) {
  std::shared_lock<std::shared_mutex> rl(e->reg_mu);
  q.needs_work = false;
  for (uint32_t p = 0; p < q.P; p++)
    if (capture_resolve_part(e, q.part[p], q.prog_ids[p])) q.needs_work = true;
}

// The two launches of an extraction: the walk per (e-mail, part), then verdict + tables.  `parts`: the PartRes the search left.
int launch_capture(zke_engine* e, CapBufs& b, const CaptureReq& q, uint32_t n, bool plain, const DfaArgs& base,
                   const uint8_t* hay_blob, const uint64_t* hay_off, const PartRes* parts, zke_result* results, hipStream_t s,
                   const LossyLaunch* lossy = nullptr) {
  const CapLayout& L = b.L;
  uint8_t* cb = b.t.d.as<uint8_t>();
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
  if (q.lossy) {
    const CapLossyArgs la{ga, ca.flags, lossy->ext_off, lossy->ext_str_off, lossy->jobs, lossy->bytes_cap};
    hipLaunchKernelGGL(capture_gather_lossy_kernel, dim3(1), dim3(1024), 0, s, la);
  } else {
    hipLaunchKernelGGL(capture_gather_kernel, dim3(1), dim3(1024), 0, s, ga);
  }
  HIPCHK(e, hipGetLastError());
  return 0;
}

// A mapped extraction's third launch, behind the two above: the origins of the body parts' spans (qpmap.hip.h), one wave per e-mail.
int launch_capture_origin(zke_engine* e, const CapBufs& b, OriginBufs& ob, const CaptureReq& q, uint32_t n, const DfaArgs& base,
                          const zke_result* results, hipStream_t s) {
  uint8_t* op = ob.t.d.as<uint8_t>();
  CapOriginArgs oa{};
  oa.n = n; oa.G = q.G; oa.gb0 = q.gbase[q.n_header_parts]; oa.d = base; oa.results = results;
  oa.spans = reinterpret_cast<const uint32_t*>(b.t.d.as<uint8_t>() + b.L.spans);
  oa.org_spans = reinterpret_cast<uint32_t*>(op); oa.org_flags = op + ob.L.flags;
  hipLaunchKernelGGL(capture_origin_kernel, dim3(n), dim3(64), 0, s, oa);
  HIPCHK(e, hipGetLastError());
  return 0;
}

// ---- the stand-alone side launches of the host entry: ONE kernel over the batch `in` (the device-side view of the packed image)
// instead of the verify pipeline, no verify workspace, the output in the side output's own buffers.
// Their common tail: zke_timings.front_end_us is the launch, the other stages are empty; the twin's first `bytes` come back as one copy.
int finish_side_launch(zke_engine* e, StageTimer& tm, const TwinBuf& t, size_t bytes, hipStream_t s) {
  HIPCHK(e, hipGetLastError());
  tm.mark(MK_FRONT); tm.mark(MK_HASH); tm.mark(MK_VERDICT);
  HIPCHK(e, t.fetch(bytes, s));
  return 0;
}
// zke_scan_signatures: the counter of selector bytes starts at zero, everything comes back
int launch_scan(zke_engine* e, ScanBufs& b, const zke_batch& in, uint64_t now, StageTimer& tm, hipStream_t s) {
  const ScanLayout& S = b.L;
  uint8_t* so = b.t.d.as<uint8_t>();
  HIPCHK(e, hipMemsetAsync(so, 0, 64, s));
  SigScanArgs sa{};
  sa.n = in.n; sa.max_sigs = S.max_sigs;
  sa.raw = in.raw_blob; sa.raw_off = in.raw_off; sa.dom = in.domain_blob; sa.dom_off = in.domain_off;
  sa.strict = e->strict; sa.now = now;
  sa.status = reinterpret_cast<uint32_t*>(so + S.status);
  sa.recs = reinterpret_cast<zke_sig_info*>(so + S.recs);
  sa.sel_blob = so + S.blob; sa.sel_cap = (uint32_t)S.blob_cap;
  sa.sel_used = reinterpret_cast<uint32_t*>(so);
  sa.hdr_ovf = b.ovf.as<uint32_t>();
  hipLaunchKernelGGL(sigscan_kernel, dim3(in.n), dim3(64), 0, s, sa);
  return finish_side_launch(e, tm, b.t, S.total, s);
}
// zke_extract_bodies: over the e-mails (the image's raw section); infos and first places come back (the second places: deliver_body)
int launch_body(zke_engine* e, BodyBufs& b, const zke_batch& in, uint32_t flags, StageTimer& tm, hipStream_t s) {
  const BodyLayout& K = b.L;
  uint8_t* bo = b.t.d.as<uint8_t>();
  const BodyArgs ba{in.n, flags, in.raw_blob, in.raw_off, reinterpret_cast<zke_body_info*>(bo), bo + K.bytes, (uint64_t)K.region, b.ovf.as<uint32_t>()};
  hipLaunchKernelGGL(body_extract_kernel, dim3(in.n), dim3(64), 0, s, ba);
  return finish_side_launch(e, tm, b.t, K.first_copy, s);
}
// zke_decode_key_records: over the records (the image's raw section); infos and keys come back
KeyrecArgs keyrec_args_of(const KeyrecBufs& b, uint32_t n, uint32_t mode, const uint8_t* blob, const uint64_t* off) {
  uint8_t* ko = b.t.d.as<uint8_t>();
  return KeyrecArgs{n, mode, blob, off, reinterpret_cast<zke_key_info*>(ko), ko + b.L.keys};
}
int launch_keyrec(zke_engine* e, KeyrecBufs& b, const zke_batch& in, uint32_t mode, StageTimer& tm, hipStream_t s) {
  const KeyrecArgs ka = keyrec_args_of(b, in.n, mode, in.raw_blob, in.raw_off);
  hipLaunchKernelGGL(keyrec_kernel, dim3(in.n), dim3(64), 0, s, ka);
  return finish_side_launch(e, tm, b.t, b.L.total, s);
}
// zke_select_keys_from_records, in front of the verify pipeline: the image's key section holds the candidates' RECORDS — decode them,
// then scan the lengths and gather the keys into the packed CSR the front end reads, which `in` points to from here on.  Three small
// launches, the keys never leave HBM.
int launch_keyrec_prefix(zke_engine* e, KeyrecBufs& b, zke_batch& in, uint32_t mode, hipStream_t s) {
  uint8_t* pk = b.pack.as<uint8_t>();
  const KeyrecArgs ka = keyrec_args_of(b, in.n, mode, in.key_blob, in.key_off);
  hipLaunchKernelGGL(keyrec_kernel, dim3(in.n), dim3(64), 0, s, ka);
  const KeyrecPackArgs pa{in.n, ka.infos, ka.keys, reinterpret_cast<uint64_t*>(pk), pk + b.L.p_type, pk + b.L.p_blob};
  hipLaunchKernelGGL(keyrec_pack_kernel, dim3(1), dim3(64), 0, s, pa);
  hipLaunchKernelGGL(keyrec_gather_kernel, dim3(in.n), dim3(64), 0, s, pa);
  HIPCHK(e, hipGetLastError());
  in.key_blob = pa.key_blob; in.key_off = pa.key_off; in.key_type = pa.key_type;
  return 0;
}

// ---- the output encoding behind a batch's records (zke_verify_emails_encoded, zke_encode_outputs; kernel: encode.hip.h): the encode
// launch over records, jobs and tables (`a`: device pointers; the outputs are filled in here from the slot's buffer), then the SHA-256
// of the encodings — the engine's hash launch over the job list the kernel left, the call sha256_batch_device_locked makes.
// `placed`: the jobs are a device plan's (capture_lossy.hip.h) and lie in the slot's buffer themselves.
int launch_encode(zke_engine* e, EncBufs& b, EncodeArgs a, hipStream_t s, bool placed = false) {
  uint8_t* eo = b.t.d.as<uint8_t>();
  a.n = b.L.n;
  a.infos = reinterpret_cast<zke_encoded_info*>(eo); a.bytes = eo + b.L.bytes; a.sha = reinterpret_cast<ShaJob*>(eo + b.L.sha);
  if (placed) hipLaunchKernelGGL(encode_outputs_placed_kernel, dim3(a.n), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(encode_outputs_kernel, dim3(a.n), dim3(64), 0, s, a);
  HIPCHK(e, hipGetLastError());
  return launch_sha(e, plan_sha(e->stage, a.n), a.sha, a.n, s);
}

// The canonicalize_signed_email pass's view of a batch whose verify pass sees B: the slot's second meta and scratch, the verify pass's
// meta to compare with, no length buckets.
BatchDev canon_pass_view(const Slot& w, const BatchDev& B) {
  BatchDev B2 = B;
  B2.meta = w.meta2.as<EmailMeta>();
  B2.scratch = w.scratch2.as<uint8_t>();
  B2.meta_verify = B.meta;
  B2.order = nullptr;
  return B2;
}

// ---- the regex stage of a mixed batch (zke_verify_emails_mixed; kernels: regex_mixed.hip.h, plan: mixed_plan.hip.h)
// (MixedLaunch, the plan of the batch and where its tables lie in the slot's staged image: host_stage.hip.h)
// Behind the verify launches: the preparation (e-mails without a config left out), ONE lane-mapped and ONE wave-mapped DFA launch
// over the plan's segments, the fold.  B: the verify pass's view of the batch; `in`: its capture tables (indexed by job).
// base_out: the launches' common DfaArgs, for the capture launches of a mixed extraction behind this stage.
int run_mixed_regex_stage(zke_engine* e, Slot& w, const BatchDev& B, const zke_batch& in, const MixedLaunch& mx, uint64_t* clean_off, uint64_t now,
                          bool want_clean, StageTimer& tm, hipStream_t s, DfaArgs* base_out = nullptr) {
  const MixedPlan& P = *mx.plan;
  const uint32_t n = B.n;
  const BatchDev B2 = canon_pass_view(w, B);
  // want_clean stays what a parity buffer asks for: whether a config has body parts is decided per e-mail (email_cfg)
  PrepMixedArgs pr{PrepArgs{ParseArgs{B2, 0, 1, 0, e->strict, now, nullptr, 0, nullptr, nullptr},
                            QpArgs{B2, B.meta, w.clean.as<uint8_t>(), clean_off, B.scratch, B.scratch_off}, want_clean ? 1u : 0u},
                   mx.email_cfg};
  hipLaunchKernelGGL(regex_prep_mixed_kernel, dim3(n), dim3(64), 0, s, pr);
  tm.mark(MK_PREP);
  DfaMixedArgs ma{};
  ma.common.b = B2;
  ma.common.scratch_v = B.scratch; ma.common.scratch_v_off = B.scratch_off;
  ma.common.clean = w.clean.as<uint8_t>(); ma.common.clean_off = clean_off;
  ma.common.cap_off = in.cap_off; ma.common.cap_str_off = in.cap_str_off; ma.common.cap_blob = in.cap_blob;
  ma.common.out = w.parts.as<PartRes>();
  ma.perm = mx.perm; ma.job_off = mx.job_off;
  if (base_out) *base_out = ma.common;
  if (P.lane_blocks) {
    ma.segs = mx.segs; ma.n_segs = P.n_lane;
    hipLaunchKernelGGL(dfa_mixed_kernel, dim3(P.lane_blocks), dim3(256), P.lane_lds, s, ma);
  }
  if (P.wave_blocks) {
    ma.segs = mx.segs + P.n_lane; ma.n_segs = (uint32_t)P.segs.size() - P.n_lane;
    hipLaunchKernelGGL(dfa_mixed_wave_kernel, dim3(P.wave_blocks), dim3(256), P.wave_lds, s, ma);
  }
  RegexFoldMixedArgs rf{B2, w.parts.as<PartRes>(), mx.job_off, mx.email_cfg};
  hipLaunchKernelGGL(regex_fold_mixed_kernel, dim3((n + 255) / 256), dim3(256), 0, s, rf);
  tm.mark(MK_DFA);
  HIPCHK(e, hipGetLastError());
  return 0;
}

// ---- capture extraction behind the mixed regex stage (zke_extract_captures_mixed; kernels: capture_mixed.hip.h)
// (CapMixedLaunch, the shape of the extraction and where its tables lie in the slot's staged image: host_stage.hip.h)
// The walk per job, then verdict + tables, as launch_capture; b.L is laid out for J jobs and Gt columns.
int launch_capture_mixed(zke_engine* e, CapBufs& b, const CapMixedLaunch& cm, uint32_t n, const DfaArgs& base, const PartRes* parts,
                         zke_result* results, hipStream_t s) {
  const CapLayout& L = b.L;
  uint8_t* cb = b.t.d.as<uint8_t>();
  CapMixedArgs ca{};
  ca.n = n; ca.J = cm.J; ca.d = base; ca.t = cm.t; ca.parts = parts;
  ca.spans = reinterpret_cast<uint32_t*>(cb + L.spans); ca.flags = cb + L.flags; ca.codes = reinterpret_cast<uint32_t*>(cb + L.codes);
  ca.work = b.work.as<uint64_t>();
  const uint32_t grid = std::min<uint32_t>(cm.J, cm.needs_work ? CAP_WORK_WAVES : 16384u);
  if (grid) hipLaunchKernelGGL(capture_mixed_kernel, dim3(grid), dim3(64), 0, s, ca);
  CapGatherMixedArgs ga{};
  ga.n = n; ga.J = cm.J; ga.Gt = cm.Gt; ga.d = base; ga.t = cm.t;
  ga.parts = parts; ga.codes = ca.codes; ga.spans = ca.spans; ga.results = results;
  ga.cap_off = reinterpret_cast<uint32_t*>(cb + L.cap_off); ga.cap_str_off = reinterpret_cast<uint32_t*>(cb + L.cap_str_off);
  ga.cap_blob = cb + L.blob; ga.blob_cap = L.blob_cap; ga.hdr = reinterpret_cast<uint64_t*>(cb + L.hdr);
  ga.tmp = reinterpret_cast<uint32_t*>(cb + L.tmp);
  hipLaunchKernelGGL(capture_gather_mixed_kernel, dim3(1), dim3(1024), 0, s, ga);
  HIPCHK(e, hipGetLastError());
  return 0;
}
int launch_capture_origin_mixed(zke_engine* e, const CapBufs& b, OriginBufs& ob, const CapMixedLaunch& cm, uint32_t n, const DfaArgs& base,
                                const zke_result* results, hipStream_t s) {
  uint8_t* op = ob.t.d.as<uint8_t>();
  CapOriginMixedArgs oa{};
  oa.n = n; oa.d = base; oa.t = cm.t; oa.results = results;
  oa.spans = reinterpret_cast<const uint32_t*>(b.t.d.as<uint8_t>() + b.L.spans);
  oa.org_spans = reinterpret_cast<uint32_t*>(op); oa.org_flags = op + ob.L.flags;
  hipLaunchKernelGGL(capture_origin_mixed_kernel, dim3(n), dim3(64), 0, s, oa);
  HIPCHK(e, hipGetLastError());
  return 0;
}

// The device pipeline.  Every pointer in `in` / out_dev is device memory, except the part-id lists (host arrays in both
// entry points).  Three launches — front end, hash / modexp stage, Ed25519 + verdict (which also runs the later signature
// rounds of the rare e-mail that needs them) — and, for verify_email_with_regex, the regex stage behind them.
// Caller holds the slot's lock; everything the call needs is in its arguments or in the slot.
int run_device_pipeline(zke_engine* e, Slot& w, const zke_batch* in, uint64_t raw_total, uint64_t key_total, zke_result* out_dev,
                        hipStream_t s, bool want_em, uint64_t now, bool want_clean = false, const CaptureReq* cap = nullptr,
                        const MixedLaunch* mixed = nullptr, const CapMixedLaunch* capmix = nullptr, const LossyLaunch* lossy = nullptr) {
  const uint32_t n = in->n;
  if (n == 0) return 0;
  const uint32_t n_pad = (n + 63) & ~63u;
  const uint32_t P = in->with_regex ? in->n_header_parts + in->n_body_parts : 0;
  int r = 0;
  if ((r = ensure_workspace(e, w, n, raw_total, in->with_regex != 0, P, want_em, s))) return r;
  // a mixed batch (with_regex, no list of its own): one PartRes per (e-mail, part) job
  if (mixed && (r = w.parts.ensure((size_t)std::max<uint32_t>(mixed->plan->shape.J, 1) * sizeof(PartRes)))) return fail(e, r, "workspace allocation");
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
  const StagePlan plan = plan_stage(e->stage, n, 4 * n_pad, key_total > (uint64_t)n * 272, B.order != nullptr, __atomic_load_n(w.wave_feedback, __ATOMIC_RELAXED));
  {
    const uint32_t round = 0;
    uint32_t* wave_count = w.pending.as<uint32_t>() + 2;
    uint32_t* wave_list = w.rsa_ok.as<uint32_t>();
    ParseArgs pa{B, round, 0, e->debug_parse_stop, e->strict, now, e->key_cache.as<KeyCacheEntry>(), plan.route_mask, wave_count, wave_list};
    // a workgroup of two waves per e-mail, the front-end wave and its helper, which canonicalises the body (parse.hip.h), where the plan says
    // that pays (stage_plan.hip.h, front_takes_helper); else one wave per e-mail
#if ZKE_PARSE_HELPER
    if (plan.front_helper) hipLaunchKernelGGL(parse_kernel<true>, dim3(n), dim3(128), 0, s, pa);
    else
#endif
    hipLaunchKernelGGL(parse_kernel<false>, dim3((n + ZKE_PARSE_WG_WAVES - 1) / ZKE_PARSE_WG_WAVES), dim3(64 * ZKE_PARSE_WG_WAVES), PARSE_DYN_LDS, s, pa);
    tm.mark(MK_FRONT);
    // hash / modexp stage: the four SHA-256 jobs and the RSA operation of every e-mail, one launch (fused.hip.h)
    if (!(e->debug_skip_launch & 1) &&
        (r = launch_hash_modexp(e, plan, B.sha, 4 * n_pad, B.rsa, n, B.meta, want_em ? w.em_dbg.as<uint8_t>() : nullptr, wave_count, wave_list, B.order, s)))
      return r;
    tm.mark(MK_HASH);
    // Ed25519 stage + verdicts (verdict.hip.h): bh compare, EM digest against the header hash, status / detail, pending counter
    EdVerdictArgs va{FinArgs{B, round, rounds, w.pending.as<uint32_t>(), e->debug_skip_rsa}, e->debug_skip_ed, wave_count,
                     e->key_cache.as<KeyCacheEntry>(), want_em ? w.em_dbg.as<uint8_t>() : nullptr, e->strict, now, w.wave_feedback};
    if (!(e->debug_skip_launch & 2)) hipLaunchKernelGGL(ed_verdict_kernel, dim3((n + VERDICT_EMAILS_PER_WAVE - 1) / VERDICT_EMAILS_PER_WAVE), dim3(64), 0, s, va);
    tm.mark(MK_VERDICT);
  }
  HIPCHK(e, hipGetLastError());

  if (in->with_regex && mixed) {
    DfaArgs base{};
    if ((r = run_mixed_regex_stage(e, w, B, *in, *mixed, clean_off, now, want_clean, tm, s, &base))) return r;
    // capture extraction (zke_extract_captures_mixed): the stage above ran without capture tables, as the single-config extraction's does
    if (capmix) {
      if ((r = launch_capture_mixed(e, w.cb, *capmix, n, base, w.parts.as<PartRes>(), out_dev, s))) return r;
      if (capmix->origin && (r = launch_capture_origin_mixed(e, w.cb, w.ob, *capmix, n, base, out_dev, s))) return r;
      tm.mark(MK_DFA);
    }
  } else if (in->with_regex) {
    // the parts of this batch, copied out of the registry (the entries themselves stay put until the engine is idle)
    PartInfo parts_small[16];
    std::vector<PartInfo> parts_big;
    PartInfo* parts = parts_small;
    if (P > 16) { parts_big.resize(P); parts = parts_big.data(); }
    {
      std::shared_lock<std::shared_mutex> rl(e->reg_mu);
      for (uint32_t p = 0; p < P; p++)
        parts[p] = part_info(e, p >= in->n_header_parts ? in->body_part_ids[p - in->n_header_parts] : in->header_part_ids[p]);
    }
    // canonicalize_signed_email (circuits.rs:34-35: first DKIM-Signature header, own scratch unless it is the verified one) and
    // remove_quoted_printable_soft_breaks (circuits.rs:37), one launch (regex.hip.h, regex_prep_kernel).  The cleaned body is
    // unobservable without body parts (circuits.rs:48-56): it is then only produced when a parity buffer asks for it.
    const BatchDev B2 = canon_pass_view(w, B);
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
      if ((r = launch_capture(e, w.cb, *cap, n, false, base, nullptr, nullptr, w.parts.as<PartRes>(), out_dev, s, lossy))) return r;
    if (cap && cap->origin_launch())
      if ((r = launch_capture_origin(e, w.cb, w.ob, *cap, n, base, out_dev, s))) return r;
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

// Which hardware queue a slot's stream sits on, read where it is visible: on the device.  HW_ID of a wave names the queue descriptor its
// dispatch packet came through — ME_ID [31:30], PIPE_ID [7:6], QUEUE_ID [26:24] — and a stream's packets all come through the descriptors of
// its one hardware queue, one per XCD.  A launch of SLOT_PROBE_GROUPS workgroups puts one on every XCD; each leaves its HW_ID in the word of
// its XCC (words 8 .. 15 of the slot's pinned block), and the host takes XCC 0's.  The other fields of the word say where the wave ran.
constexpr uint32_t SLOT_PROBE_GROUPS = 64;
constexpr uint32_t SLOT_PROBE_WORD0 = 8;               // first of the eight words, in uint32_t of Slot::wave_feedback
constexpr uint32_t SLOT_PROBE_UNWRITTEN = 0xFFFFFFFFu; // no HW_ID reads all ones: ME_ID 3 does not exist
constexpr uint32_t SLOT_PROBE_QUEUE_MASK = (3u << 30) | (7u << 24) | (3u << 6);
__global__ void slot_queue_probe_kernel(uint32_t* block) {
  if (threadIdx.x != 0) return;
  const uint32_t hw_id = __builtin_amdgcn_s_getreg(4 | (31 << 11));
  const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11)) & 7u;          // XCC_ID [3:0]; eight words: the index stays inside the block
  __hip_atomic_store(block + SLOT_PROBE_WORD0 + xcc, hw_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Rebuild the engine's ticket order from the hardware queues its slot streams sit on (under `big` exclusive, every slot stream idle and
// its hardware queue in being: no queue is created while the probes run).  A map that does not come out — a word not written, more
// queues than the pool has, a queue per slot — leaves the order at plain round-robin (slot_order_build).
int probe_slot_queues(zke_engine* e) {
  const uint32_t S = (uint32_t)e->slots.size();
  slot_order_unknown(e->order, S);
  for (Slot* w : e->slots) {
    for (uint32_t k = 0; k < 8; k++) w->wave_feedback[SLOT_PROBE_WORD0 + k] = SLOT_PROBE_UNWRITTEN;
    hipLaunchKernelGGL(slot_queue_probe_kernel, dim3(SLOT_PROBE_GROUPS), dim3(64), 0, w->stream, w->wave_feedback);
  }
  HIPCHK(e, hipGetLastError());
  for (Slot* w : e->slots) HIPCHK(e, hipStreamSynchronize(w->stream));
  uint32_t id[SLOT_ORDER_MAX_SLOTS];
  uint8_t known[SLOT_ORDER_MAX_SLOTS];
  for (uint32_t s = 0; s < S; s++) {
    const uint32_t word = __atomic_load_n(e->slots[s]->wave_feedback + SLOT_PROBE_WORD0, __ATOMIC_RELAXED);
    known[s] = word != SLOT_PROBE_UNWRITTEN;
    id[s] = word & SLOT_PROBE_QUEUE_MASK;
  }
  (void)slot_order_build(e->order, id, known, S, e->stage.hw_queues);
#ifdef ZKE_DEV_KNOBS
  if (getenv("ZKE_DEBUG_QUEUE_PROBE")) {          // the raw words, for profiles/queue_balance_queues.txt
    for (uint32_t s = 0; s < S; s++) {
      fprintf(stderr, "queue_probe slot %2u group %2d HW_ID by XCC:", s, e->order.n_queues ? (int)e->order.queue_of[s] : -1);
      for (uint32_t k = 0; k < 8; k++) fprintf(stderr, " %08x", e->slots[s]->wave_feedback[SLOT_PROBE_WORD0 + k]);
      fprintf(stderr, "\n");
    }
  }
#endif
  return 0;
}

// The slot's next submission ticket: round-robin over the hardware queues the slot streams share and over a queue's slots within it, or,
// with the map unknown, over the slots that exist (slot_order.hip.h; zke_engine_reserve only appends).
Slot& next_slot(zke_engine* e, uint32_t& index, uint64_t* ticket_no = nullptr) {
  const uint64_t t = e->ticket.fetch_add(1, std::memory_order_relaxed);
  if (ticket_no) *ticket_no = t;
  index = slot_for_ticket(e->order, t);
  e->last_slot.store(index, std::memory_order_relaxed);
  return *e->slots[index];
}
// tickets: slot index in the low 6 bits (an engine has at most 64 slots), the slot's batch count above
inline uint64_t make_ticket(uint32_t slot, uint64_t gen) { return (gen << 6) | slot; }

uint64_t batch_clock(const zke_engine* e) {
  if (!(e->strict & ZKE_STRICT_EXPIRY_X)) return 0;
  return e->opt.now_unix ? e->opt.now_unix : (uint64_t)time(nullptr);
}

}  // namespace

extern "C" {

int zke_engine_reserve(zke_engine* e, uint32_t max_n, uint64_t max_raw_total, uint32_t slots, uint32_t max_regex_parts) {
  if (!e || slots == 0 || slots > 64) return ZKE_E_ARG;
  std::unique_lock<std::shared_mutex> ex(e->big);
  HIPCHK(e, hipSetDevice(e->device));
  while (e->slots.size() < slots) {
    Slot* w = new_slot(e);
    if (!w) return ZKE_E_DEVICE;
    e->slots.push_back(w);
    e->stage.slots = (uint32_t)e->slots.size();
  }
  if (e->order.slots != e->slots.size()) slot_order_unknown(e->order, (uint32_t)e->slots.size());      // until the probe below has run
  if (max_n)
    for (Slot* w : e->slots)
      if (int r = ensure_workspace(e, *w, max_n, max_raw_total, max_regex_parts != 0, max_regex_parts, false, w->stream)) return r;
  if (max_n && max_regex_parts)          // the capture workspace: four groups of 32 bytes per part is what a larger extraction regrows from
    for (Slot* w : e->slots)
      if (int r = ensure_capture_buffers(e, w->cb, cap_layout(max_n, max_regex_parts, 4 * max_regex_parts, (size_t)max_n * max_regex_parts * 128), true)) return r;

  // A stream's hardware queue and the queue's scratch memory (the front end spills a few registers) come into being
  // with the first launch that needs them — milliseconds, and they would land in the first batch of every slot.
  // One trivial launch per slot, with more scratch per lane than any kernel of the pipeline, pays for both here.
  // Then one empty e-mail through the whole pipeline of every slot: kernel code, kernel arguments and the slot's workspace
  // pages have all been touched once before the first real batch arrives.
  if (int r = e->misc.ensure(1024)) return fail(e, r, "workspace allocation");
  HIPCHK(e, hipMemsetAsync(e->misc.p, 0, 1024, e->stream));      // every slot's warm-up batch below reads these zeros: they are there
  HIPCHK(e, hipStreamSynchronize(e->stream));                    // before the first of them is launched (see ensure_zeroed)
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
  if (int r = probe_slot_queues(e)) return r;          // every slot stream has its hardware queue now: which of them share one
  if (e->host_image_cap.load())          // slots created just now get the staging the others have (everything is drained: see grow_host_staging)
    for (Slot* w : e->slots)
      if (int r = ensure_host_buffers(e, *w, e->host_image_cap.load(), e->host_n_cap.load())) return r;
  return 0;
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

}  // extern "C"
