// mixed_plan.hip.h — the host plan of a mixed regex batch (zke_verify_emails_mixed): `&[EmailWithRegex]` whose values carry
// different RegexInfo (core/src/structs.rs:32-35,59-62; core/src/circuits.rs:31-68 takes them one at a time, so a slice of them is
// heterogeneous by construction).  A pure function of config_of[n], the configs' part counts, the parts as the registry resolved
// them and the mapping rule: no HIP call, no engine state — it compiles as plain C++ (tests/cpp/mixed_plan_fuzz.cpp).
//
//   job_off[n + 1]   prefix sum of P(config_of[i]) (0 for ZKE_CONFIG_NONE): e-mail i's part p is job job_off[i] + p, header parts
//                    first — the index of its PartRes and of its entry in the capture table;
//   email_cfg[n]     what the per-e-mail kernels need of the e-mail's config: MIXED_CFG_NONE, or n_header_parts with
//                    MIXED_CFG_HAS_BODY or-ed in;
//   perm[m]          the e-mails that have a config, grouped by config, in their order within each (a stable counting sort);
//   segs[S]          one segment per (config, part): which automaton, which range of perm, which blocks of which launch.
//                    S depends on the configs alone (at most ZKE_MIXED_MAX_CONFIGS x ZKE_MIXED_MAX_PARTS), never on n.
// The lane-mapped launch (one e-mail per lane, 256 per block) holds the segments [0, n_lane), the wave-mapped launch (one e-mail
// per wave, 4 per block) the segments [n_lane, S); inside a launch the segments' block ranges follow each other without a gap, and
// a block finds its segment by a binary search for the first block_end beyond its index.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zke {

constexpr uint32_t MIXED_MAX_CONFIGS = 64;           // = ZKE_MIXED_MAX_CONFIGS
constexpr uint32_t MIXED_MAX_PARTS = 64;             // = ZKE_MIXED_MAX_PARTS: header + body parts of one config
constexpr uint32_t MIXED_NONE = 0xFFFFFFFFu;         // = ZKE_CONFIG_NONE
constexpr uint32_t MIXED_CFG_NONE = 0xFFFFFFFFu;     // email_cfg: the e-mail is verify_email only
constexpr uint32_t MIXED_CFG_HAS_BODY = 1u << 16;    // email_cfg: its config has body parts (somebody reads the cleaned body)
constexpr uint32_t MIXED_CFG_NH_MASK = 0xFFFFu;
constexpr size_t MIXED_LDS_CAP = 150 * 1024;         // the DFA launches' cap on dynamic LDS (pipeline.hip.h, part_lds)
constexpr uint32_t MIXED_LANE_BLOCK = 256, MIXED_WAVE_BLOCK = 4;      // e-mails per block of the two launches

struct MixedConfigIn { uint32_t n_header_parts, n_body_parts; };
// One part of one config as the registry resolved it (PartInfo), config-major, header parts first.
struct MixedPartIn {
  uint64_t dev;            // device address of the RegexDev; 0: the pair does not deserialise / the id is not registered
  size_t lds_bytes;        // repacked fwd + rev tables
  uint32_t idle;           // the forward automaton's idle state (~0: none)
  uint32_t detail;         // dev == 0: the ZKE_D_DFA_* section
};
// Device image of one segment (48 bytes; read by the blocks of dfa_mixed_kernel / dfa_mixed_wave_kernel).
struct MixedSeg {
  uint64_t re;             // device address of the RegexDev, or 0 ...
  uint32_t decode_detail;  // ... and why
  uint32_t part;           // index within the config's list, header parts first
  uint32_t is_body;
  uint32_t lds_tables;     // 1: both tables are staged in the launch's dynamic LDS; 0: walked from HBM
  uint32_t idle;           // wave launch: the idle state of the clean-chunk pre-pass (~0: none); lane launch: ~0
  uint32_t first, count;   // perm[first, first + count): the config's e-mails
  uint32_t block0;         // first block of the segment in its launch
  uint32_t block_end;      // one past its last block (== block0: no e-mail has this config)
  uint32_t config;
};
static_assert(sizeof(MixedSeg) == 48, "MixedSeg is a device image");

struct MixedShape { uint32_t m = 0, J = 0, n_segs = 0; bool any_body = false; };
struct MixedPlan {
  MixedShape shape;
  std::vector<uint32_t> job_off, email_cfg, perm;
  std::vector<uint32_t> cfg_first;       // [n_configs + 1]: config c's e-mails are perm[cfg_first[c], cfg_first[c + 1])
  std::vector<MixedSeg> segs;
  uint32_t n_lane = 0;                   // segs[0, n_lane): lane launch; the rest: wave launch
  uint32_t lane_blocks = 0, wave_blocks = 0;
  size_t lane_lds = 1024, wave_lds = 1024;   // dynamic LDS of the two launches: the largest need among their segments that have blocks
};

// What a segment needs of the launch's dynamic LDS, and whether its tables go there (the rule of pipeline.hip.h's part_lds).
inline size_t mixed_part_lds(const MixedPartIn& p, uint32_t& in_lds) {
  in_lds = 0;
  if (p.dev && p.lds_bytes + 1024 <= MIXED_LDS_CAP) { in_lds = 1; return p.lds_bytes + 1024; }
  return 1024;
}
// The first part that is wave-mapped in a config with nh header parts and P parts.  The rule is the single-config one, decided on
// the batch's n: mapping 1 forces lanes, 2 waves; else up to 1 024 e-mails everything is wave-mapped, above that the body parts.
inline uint32_t mixed_wave_from(uint32_t mapping, uint32_t n, uint32_t nh, uint32_t P) {
  return mapping == 1 ? P : mapping == 2 ? 0u : (n <= 1024 ? 0u : nh);
}

// The checks, and the sizes that follow from the arguments alone.  0, or a message (nothing has been written).
inline const char* mixed_plan_check(const uint32_t* config_of, uint32_t n, const MixedConfigIn* cfgs, uint32_t n_configs, MixedShape& out) {
  if (n_configs > MIXED_MAX_CONFIGS) return "more than ZKE_MIXED_MAX_CONFIGS configs";
  if ((n_configs && !cfgs) || (n && !config_of)) return "null pointer";
  uint32_t P[MIXED_MAX_CONFIGS];
  MixedShape s;
  for (uint32_t c = 0; c < n_configs; c++) {
    if (cfgs[c].n_header_parts > MIXED_MAX_PARTS || cfgs[c].n_body_parts > MIXED_MAX_PARTS - cfgs[c].n_header_parts)
      return "more than ZKE_MIXED_MAX_PARTS parts in a config";
    P[c] = cfgs[c].n_header_parts + cfgs[c].n_body_parts;
    s.n_segs += P[c];
    s.any_body = s.any_body || cfgs[c].n_body_parts != 0;
  }
  uint64_t J = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t c = config_of[i];
    if (c == MIXED_NONE) continue;
    if (c >= n_configs) return "config_of names no config (neither below n_configs nor ZKE_CONFIG_NONE)";
    s.m++; J += P[c];
  }
  if (J >= (1ull << 31)) return "2^31 (e-mail, part) jobs or more: split the batch";
  s.J = (uint32_t)J;
  out = s;
  return nullptr;
}

// The plan.  `parts`: [shape.n_segs], config-major.  0, or the message of mixed_plan_check — then `out` is as it was.
inline const char* mixed_plan_build(const uint32_t* config_of, uint32_t n, const MixedConfigIn* cfgs, uint32_t n_configs, const MixedPartIn* parts,
                                    uint32_t mapping, MixedPlan& out) {
  MixedShape shape;
  if (const char* why = mixed_plan_check(config_of, n, cfgs, n_configs, shape)) return why;
  if (shape.n_segs && !parts) return "null pointer";
  out.shape = shape;
  out.job_off.assign((size_t)n + 1, 0);
  out.email_cfg.assign(n, MIXED_CFG_NONE);
  out.perm.assign(shape.m, 0);
  out.cfg_first.assign((size_t)n_configs + 1, 0);
  // counting sort by config, stable; the prefix sum of P along the way
  for (uint32_t i = 0; i < n; i++) if (config_of[i] != MIXED_NONE) out.cfg_first[config_of[i] + 1]++;
  for (uint32_t c = 0; c < n_configs; c++) out.cfg_first[c + 1] += out.cfg_first[c];
  {
    uint32_t cursor[MIXED_MAX_CONFIGS];
    for (uint32_t c = 0; c < n_configs; c++) cursor[c] = out.cfg_first[c];
    uint32_t j = 0;
    for (uint32_t i = 0; i < n; i++) {
      out.job_off[i] = j;
      const uint32_t c = config_of[i];
      if (c == MIXED_NONE) continue;
      out.perm[cursor[c]++] = i;
      out.email_cfg[i] = cfgs[c].n_header_parts | (cfgs[c].n_body_parts ? MIXED_CFG_HAS_BODY : 0u);
      j += cfgs[c].n_header_parts + cfgs[c].n_body_parts;
    }
    out.job_off[n] = j;
  }
  // the segments: the lane launch's first, then the wave launch's; config-major inside each
  out.segs.clear();
  out.segs.reserve(shape.n_segs);
  out.lane_lds = out.wave_lds = 1024;
  out.lane_blocks = out.wave_blocks = 0;
  for (int wave = 0; wave < 2; wave++) {
    uint32_t block = 0;
    size_t lds = 1024;
    const uint32_t per_block = wave ? MIXED_WAVE_BLOCK : MIXED_LANE_BLOCK;
    uint32_t base = 0;                       // of config c's parts in `parts`
    for (uint32_t c = 0; c < n_configs; c++) {
      const uint32_t nh = cfgs[c].n_header_parts, P = nh + cfgs[c].n_body_parts;
      const uint32_t wave_from = mixed_wave_from(mapping, n, nh, P);
      const uint32_t first = out.cfg_first[c], count = out.cfg_first[c + 1] - first;
      for (uint32_t p = 0; p < P; p++) {
        if ((p >= wave_from) != (wave != 0)) continue;
        const MixedPartIn& pi = parts[base + p];
        MixedSeg s{};
        s.re = pi.dev; s.decode_detail = pi.detail; s.part = p; s.is_body = p >= nh ? 1u : 0u;
        const size_t need = mixed_part_lds(pi, s.lds_tables);
        s.idle = (pi.dev && wave) ? pi.idle : 0xFFFFFFFFu;
        s.first = first; s.count = count; s.config = c;
        s.block0 = block;
        block += (count + per_block - 1) / per_block;
        s.block_end = block;
        if (count && need > lds) lds = need;
        out.segs.push_back(s);
      }
      base += P;
    }
    if (wave) { out.wave_blocks = block; out.wave_lds = lds; }
    else { out.lane_blocks = block; out.lane_lds = lds; out.n_lane = (uint32_t)out.segs.size(); }
  }
  return nullptr;
}

// The plan's section of the staged image: job_off | email_cfg | perm | segs, each 16-byte aligned.
struct MixedImage { size_t job_off, email_cfg, perm, segs, total; };
inline MixedImage mixed_image(uint32_t n, const MixedShape& s) {
  MixedImage L{};
  size_t o = 0;
  auto put = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~(size_t)15; return at; };
  L.job_off = put(((size_t)n + 1) * 4);
  L.email_cfg = put((size_t)n * 4);
  L.perm = put((size_t)s.m * 4);
  L.segs = put((size_t)s.n_segs * sizeof(MixedSeg));
  L.total = o;
  return L;
}

// ---- what a mixed EXTRACTION needs on top of that (zke_extract_captures_mixed; kernels: capture_mixed.hip.h).  The verify plan above is
// built as for zke_verify_emails_mixed from the same config_of and the configs' part counts; this half adds the ragged columns:
//   col_off[n + 1]   prefix sum of G(config_of[i]), the requested groups of the e-mail's config (0 for ZKE_CONFIG_NONE): requested
//                    group k of the e-mail's part p is column col_off[i] + gbase[p] + k, gbase the prefix sum of the config's
//                    per-part group counts;
//   cap_cfg[n]       the e-mail's config index, or MIXED_NONE — a job is mapped to its e-mail by a binary search of job_off, the
//                    e-mail to its config by this word;
//   cfgs[n_configs]  per config {first part in the config-major part table, n_header_parts, G, first body column};
//   gbase[n_parts]   per entry of the part table the first column of the part among its config's G.
// Like the plan above a pure function: every check precedes the first write.
constexpr uint32_t CAPMIX_MAX_PARTS = 16;            // = ZKE_CAP_MAX_PARTS: parts of one config of an extraction
constexpr uint32_t CAPMIX_MAX_GROUPS = 16;           // = ZKE_CAP_MAX_GROUPS: groups requested of one part
constexpr uint64_t CAPMIX_MAX_COLUMNS = 1ull << 20;  // Gt * ZKE_CAP_MAX_SPAN must stay below 4 GiB (32-bit string offsets)

struct CapMixedCfg { uint32_t part0, nh, G, gb0; };  // device image, 16 bytes
static_assert(sizeof(CapMixedCfg) == 16, "CapMixedCfg is a device image");
struct CapMixedShape { uint32_t J = 0, Gt = 0, n_parts = 0; bool body_groups = false; };   // body_groups: some body part asks for a group
struct CapMixedPlan {
  CapMixedShape shape;
  std::vector<uint32_t> col_off, cap_cfg, gbase;
  std::vector<CapMixedCfg> cfgs;
};

// `groups`: the requested-group count of every part, config-major, header parts first (the sum of the configs' part counts entries).
// 0, or a message (nothing has been written).
inline const char* capmix_plan_check(const uint32_t* config_of, uint32_t n, const MixedConfigIn* cfgs, uint32_t n_configs, const uint32_t* groups,
                                     CapMixedShape& out) {
  if (n_configs > MIXED_MAX_CONFIGS) return "more than ZKE_MIXED_MAX_CONFIGS configs";
  if ((n_configs && !cfgs) || (n && !config_of)) return "null pointer";
  uint32_t P[MIXED_MAX_CONFIGS], G[MIXED_MAX_CONFIGS];
  CapMixedShape s;
  for (uint32_t c = 0; c < n_configs; c++) {
    if (cfgs[c].n_header_parts > CAPMIX_MAX_PARTS || cfgs[c].n_body_parts > CAPMIX_MAX_PARTS - cfgs[c].n_header_parts ||
        cfgs[c].n_header_parts + cfgs[c].n_body_parts == 0)
      return "a config needs 1 .. ZKE_CAP_MAX_PARTS parts (ZKE_CONFIG_NONE is the way to say: no regex)";
    P[c] = cfgs[c].n_header_parts + cfgs[c].n_body_parts;
    if (!groups) return "null pointer";
    G[c] = 0;
    for (uint32_t p = 0; p < P[c]; p++) {
      const uint32_t g = groups[s.n_parts + p];
      if (g > CAPMIX_MAX_GROUPS) return "more than ZKE_CAP_MAX_GROUPS groups requested for a part";
      G[c] += g;
      if (p >= cfgs[c].n_header_parts && g) s.body_groups = true;
    }
    s.n_parts += P[c];
  }
  uint64_t J = 0, Gt = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t c = config_of[i];
    if (c == MIXED_NONE) continue;
    if (c >= n_configs) return "config_of names no config (neither below n_configs nor ZKE_CONFIG_NONE)";
    J += P[c]; Gt += G[c];
  }
  if (Gt >= CAPMIX_MAX_COLUMNS)
    return "requested groups beyond what 32-bit string offsets address (their sum over the e-mails times ZKE_CAP_MAX_SPAN must stay below 4 GiB): split the batch";
  if (J >= (1ull << 31)) return "2^31 (e-mail, part) jobs or more: split the batch";
  s.J = (uint32_t)J; s.Gt = (uint32_t)Gt;
  out = s;
  return nullptr;
}

// 0, or the message of capmix_plan_check — then `out` is as it was.
inline const char* capmix_plan_build(const uint32_t* config_of, uint32_t n, const MixedConfigIn* cfgs, uint32_t n_configs, const uint32_t* groups,
                                     CapMixedPlan& out) {
  CapMixedShape shape;
  if (const char* why = capmix_plan_check(config_of, n, cfgs, n_configs, groups, shape)) return why;
  out.shape = shape;
  out.cfgs.assign(n_configs, CapMixedCfg{});
  out.gbase.assign(shape.n_parts, 0);
  uint32_t part0 = 0;
  for (uint32_t c = 0; c < n_configs; c++) {
    const uint32_t nh = cfgs[c].n_header_parts, P = nh + cfgs[c].n_body_parts;
    uint32_t g = 0, gb0 = 0;
    for (uint32_t p = 0; p < P; p++) {
      if (p == nh) gb0 = g;
      out.gbase[part0 + p] = g;
      g += groups[part0 + p];
    }
    if (nh == P) gb0 = g;
    out.cfgs[c] = CapMixedCfg{part0, nh, g, gb0};
    part0 += P;
  }
  out.col_off.assign((size_t)n + 1, 0);
  out.cap_cfg.assign(n, MIXED_NONE);
  uint32_t col = 0;
  for (uint32_t i = 0; i < n; i++) {
    out.col_off[i] = col;
    const uint32_t c = config_of[i];
    if (c == MIXED_NONE) continue;
    out.cap_cfg[i] = c;
    col += out.cfgs[c].G;
  }
  out.col_off[n] = col;
  return nullptr;
}

// Its section of the staged image, behind the verify plan's: col_off | cap_cfg | cfgs | the part table (part_bytes per entry: the
// device's CapPartDev, resolved against the registry when the batch is submitted), each 16-byte aligned.
struct CapMixedImage { size_t col_off, cap_cfg, cfgs, parts, total; };
inline CapMixedImage capmix_image(uint32_t n, uint32_t n_configs, const CapMixedShape& s, size_t part_bytes) {
  CapMixedImage L{};
  size_t o = 0;
  auto put = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~(size_t)15; return at; };
  L.col_off = put(((size_t)n + 1) * 4);
  L.cap_cfg = put((size_t)n * 4);
  L.cfgs = put((size_t)n_configs * sizeof(CapMixedCfg));
  L.parts = put((size_t)s.n_parts * part_bytes);
  L.total = o;
  return L;
}

}  // namespace zke
