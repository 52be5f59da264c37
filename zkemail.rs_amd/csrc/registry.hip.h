// registry.hip.h — the engine's registries: parsed DFA pairs (zke_dfa_*; lookup, LRU eviction, pins) and capture programs
// (zke_capture_*); parsers and entry types: dfa_registry.hip.h.  One parse per distinct pair replaces the per-e-mail
// dense::DFA::from_bytes of core/src/regex.rs:32-33.  Included by engine.hip behind zke_engine's definition (single translation unit).
#pragma once

namespace {

// (caller holds reg_mu exclusively or is creating the engine)
int raise_dfa_lds_attrs(zke_engine* e, size_t lds) {
  // (each mapping's two kernels together: the single-config launch and the mixed batch's, regex_mixed.hip.h)
  if (lds > e->dfa_wave_lds_attr) {
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&dfa_wave_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&dfa_mixed_wave_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    e->dfa_wave_lds_attr = lds;
  }
  if (lds > e->dfa_lds_attr) {
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&dfa_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&dfa_mixed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    e->dfa_lds_attr = lds;
  }
  return 0;
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

}  // extern "C"
