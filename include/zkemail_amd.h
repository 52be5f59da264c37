/*
 * zkemail_amd.h — C-ABI of the MI355X-native batched email-verification engine.
 *
 * This is the drop-in boundary for zkemail_core's two public functions
 *
 *     pub fn verify_email(email: &Email) -> EmailVerifierOutput             (core/src/circuits.rs:9)
 *     pub fn verify_email_with_regex(input: &EmailWithRegex)
 *                                   -> EmailWithRegexVerifierOutput         (core/src/circuits.rs:31)
 *
 * The reference has no FFI of its own; these entry points are what a
 * Rust `-sys` shim for that path binds (INTEGRATION.md shows the `extern "C"` block).
 * Plain pointers and sizes only; no C++ or torch types.
 *
 * All multi-byte integers are host-endian (little-endian on the target).  Offsets
 * arrays are CSR style: entry i spans blob[off[i] .. off[i+1]).
 *
 * Failure model.  The reference panics (process abort under its release profile,
 * Cargo.toml:35).  A batch engine must not abort a batch, so every email gets a
 * `status` naming the reference panic site that would have fired.  The C++ mirror in
 * include/zkemail_core.hpp re-raises them to keep drop-in semantics.
 */
#ifndef ZKEMAIL_AMD_H
#define ZKEMAIL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status codes */
/* One per reference panic site. */
enum {
  ZKE_OK                  = 0,
  ZKE_PARSE_FAIL          = 1,  /* mailparse::parse_mail(..).unwrap()            core/src/email.rs:26 */
  ZKE_KEY_DECODE_FAIL     = 2,  /* DkimPublicKey::try_from_bytes(..).unwrap()    core/src/email.rs:29 */
  ZKE_DKIM_ERROR          = 3,  /* verify_email_with_key(..).unwrap()            core/src/email.rs:33 */
  ZKE_DKIM_NOT_PASS       = 4,  /* assert!(verified)                             core/src/circuits.rs:13 */
  ZKE_EXTERNAL_INPUT_NULL = 5,  /* .expect("Value cannot be null")               core/src/circuits.rs:24 */
  ZKE_CANON_FAIL          = 6,  /* canonicalize_signed_email(..).unwrap()        core/src/circuits.rs:35 */
  ZKE_DFA_DECODE_FAIL     = 7,  /* dense::DFA::from_bytes(..).unwrap()           core/src/regex.rs:32-33 */
  ZKE_HEADER_REGEX_FAIL   = 8,  /* assert!(verified) on header parts             core/src/circuits.rs:45 */
  ZKE_BODY_REGEX_FAIL     = 9,  /* assert!(verified) on body parts               core/src/circuits.rs:54 */
  ZKE_UNSUPPORTED         = 10, /* input is outside what this engine implements; never a silent mis-verify */
  ZKE_BODY_DECODE_FAIL    = 11  /* part.get_body_raw().unwrap() in extract_email_body (zke_extract_bodies only)  core/src/email.rs:17-21 */
};

/* `detail` sub-codes.  For ZKE_DKIM_NOT_PASS they mirror cfdkim's DKIMError of the
 * last signature tried (the text after "fail (" in DKIMResult::with_detail()). */
enum {
  ZKE_D_NONE                 = 0,
  ZKE_D_NEUTRAL              = 1,  /* no DKIM-Signature with d= == from_domain was tried */
  ZKE_D_SIG_SYNTAX           = 2,  /* tag-list did not parse */
  ZKE_D_MISSING_TAG          = 3,  /* one of v a b bh d h s absent */
  ZKE_D_INCOMPATIBLE_VERSION = 4,  /* v != "1" */
  ZKE_D_DOMAIN_MISMATCH      = 5,  /* i= does not end with d= */
  ZKE_D_FROM_NOT_SIGNED      = 6,  /* h= lacks "from" */
  ZKE_D_BAD_QUERY_METHOD     = 7,  /* q= present and != "dns/txt" */
  ZKE_D_BAD_CANON            = 8,  /* c= not one of the six accepted spellings */
  ZKE_D_BAD_ALGO             = 9,  /* a= not rsa-sha1 / rsa-sha256 / ed25519-sha256 */
  ZKE_D_BAD_LENGTH           = 10, /* l= not a decimal usize */
  ZKE_D_BODY_HASH_MISMATCH   = 11, /* base64(SHA-256(canon body)) != bh= */
  ZKE_D_SIG_B64              = 12, /* b= is not canonical padded base64 */
  ZKE_D_SIG_MISMATCH         = 13, /* RSASSA-PKCS1-v1_5 / Ed25519 verification failed (an Ed25519 b= that is not 64 bytes included) */
  /* ZKE_PARSE_FAIL */
  ZKE_D_HDR_LEADING_SPACE    = 20, /* header line starts with ' ' */
  ZKE_D_HDR_LONE_CR          = 21, /* headers followed by a lone CR */
  ZKE_D_EMPTY_INPUT          = 22,
  ZKE_D_SUBPART_LEADING_SPACE = 23, /* the same two errors in the header block of a MIME subpart (parse_mail walks the multipart tree) */
  ZKE_D_SUBPART_LONE_CR      = 24,
  /* ZKE_KEY_DECODE_FAIL */
  ZKE_D_KEY_TYPE             = 30, /* key_type not "rsa"/"ed25519" */
  ZKE_D_KEY_DER              = 31, /* not a DER RSAPublicKey */
  ZKE_D_KEY_RANGE            = 32, /* modulus > 4096 bits, e < 2 or e > 2^33-1 */
  ZKE_D_KEY_ED25519_POINT    = 33, /* 32-byte Ed25519 key is not a curve point (VerifyingKey::from_bytes fails) */
  /* ZKE_CANON_FAIL */
  ZKE_D_NO_SIGNATURE         = 40, /* no DKIM-Signature header at all */
  /* ZKE_UNSUPPORTED */
  ZKE_D_U_ALGO_SHA1          = 50, /* (unused since a=rsa-sha1 is implemented) */
  ZKE_D_U_ALGO_ED25519       = 51, /* a= and key type disagree (a=ed25519-sha256 with an RSA key, a=rsa-* with an Ed25519
                                      key): cfdkim errors or verifies against the key type; reported, never guessed */
  ZKE_D_U_SIG_NON_ASCII      = 52, /* DKIM-Signature value has bytes >= 0x80 (reference goes through from_utf8_lossy) */
  ZKE_D_U_TOO_MANY_HEADERS   = 53, /* more than ZKE_MAX_HEADERS header fields */
  ZKE_D_U_PREIMAGE_OVERFLOW  = 54, /* canonicalised header preimage exceeds its scratch slot */
  ZKE_D_U_EVEN_MODULUS       = 55,
  ZKE_D_U_TOO_MANY_TAGS      = 56,
  ZKE_D_U_CAPTURE_FFFD       = 57, /* capture holds U+FFFD and the match text is not valid UTF-8 */
  ZKE_D_U_EMAIL_TOO_LARGE    = 58, /* raw email >= 2^31 bytes */
  /* regex */
  ZKE_D_RE_MATCH_COUNT       = 60, /* find_iter(..).count() != 1      core/src/regex.rs:37 */
  ZKE_D_RE_CAPTURE_MISSING   = 61, /* !matched_str.contains(capture)  core/src/regex.rs:44 */
  ZKE_D_RE_QUIT              = 62, /* DFA entered its quit state (find_iter panics in the reference) */
  /* ZKE_UNSUPPORTED, continued */
  ZKE_D_U_SIG_TOO_LONG       = 63, /* FWS-stripped tag values of one DKIM-Signature exceed ZKE_MAX_TAGBUF bytes */
  ZKE_D_U_TOO_MANY_SIGS      = 64, /* more failing same-domain signatures than the engine's signature rounds */
  ZKE_D_U_SIG_B_REPEATED     = 65, /* (no longer produced: both front ends remove every occurrence of the raw b= value, as the reference does) */
  ZKE_D_U_DOMAIN_FOLD        = 66, /* from_domain holds U+212A KELVIN SIGN, the one non-ASCII character whose to_lowercase() is ASCII ("k"):
                                      cfdkim compares d= and from_domain lower-cased as Unicode strings; the engine folds ASCII only,
                                      which is exact for every other domain (d= itself is ASCII whenever it gets that far) */
  ZKE_D_U_MIME_CTYPE         = 67, /* a Content-Type value that decides the subpart walk holds bytes >= 0x80 or an RFC 2047 encoded word */
  ZKE_D_U_MIME_BOUNDARY      = 68, /* multipart boundary parameter folded across lines, or given only in an RFC 2231 form (boundary*, boundary*0) */
  ZKE_D_U_MIME_DEPTH         = 69, /* multiparts nested more than 8 deep */
  /* ZKE_DKIM_NOT_PASS, continued */
  ZKE_D_SIG_EXPIRED          = 14, /* x= lies in the past (only with zke_options.enforce_expiry_x) */
  /* ZKE_DFA_DECODE_FAIL: the section of the regex-automata dense-DFA blob at which dense::DFA::from_bytes would have
   * given up (core/src/regex.rs:32-33).  70..79: the forward blob (verify_re.fwd); + 10: the reverse blob (verify_re.bwd).
   * The sections the committed regex-automata blobs do not pin (unanchored start block, accelerators, quit set)
   * have codes of their own so that the first real blob that fails says where the recalled layout is wrong. */
  ZKE_D_DFA_LABEL            = 70, /* label / padding ("rust-regex-automata-dfa-dense\0", NUL-padded to 32 bytes) */
  ZKE_D_DFA_ENDIAN_VERSION   = 71, /* endianness marker 0x0000FEFF, version 2, the unused word */
  ZKE_D_DFA_FLAGS            = 72, /* the flags word */
  ZKE_D_DFA_TRANSITIONS      = 73, /* state_len, stride2, byte classes, the transition table and its ids */
  ZKE_D_DFA_START_TABLE      = 74, /* start kind, start-byte map, stride, pattern_len, universal starts, the start ids */
  ZKE_D_DFA_MATCH_STATES     = 75, /* match-state slices, pattern_len, pattern ids */
  ZKE_D_DFA_SPECIAL          = 76, /* the eight special-state bounds */
  ZKE_D_DFA_ACCELS           = 77, /* accelerator count and records */
  ZKE_D_DFA_QUITSET          = 78, /* the 256-bit quit set */
  ZKE_D_DFA_UNREGISTERED     = 79, /* the part id names no registered pair (never registered, or unregistered since) */
  /* capture extraction (zke_extract_captures, zke_capture_batch): helpers/src/regex.rs:16-51 */
  ZKE_D_RE_GROUP_MISSING     = 90, /* a requested group is not in the pattern or took no part in the match ("Capture group not found",
                                      helpers/src/regex.rs:31); status ZKE_HEADER_REGEX_FAIL / ZKE_BODY_REGEX_FAIL */
  /* ZKE_UNSUPPORTED, continued */
  ZKE_D_U_CAPTURE_STATES     = 91, /* the capture program has more than ZKE_CAP_MAX_STATES states or ZKE_CAP_MAX_PROGRAM_GROUPS groups */
  ZKE_D_U_CAPTURE_SPAN       = 92, /* the match is longer than ZKE_CAP_MAX_SPAN bytes */
  ZKE_D_U_CAPTURE_WALK       = 93, /* the capture program cannot reproduce the span its DFA pair found (the two were not compiled
                                      from one pattern, or the walk met a case it does not implement): reported, never guessed */
  ZKE_D_U_CAPTURE_PROGRAM    = 94, /* the capture program does not decode, or its id is not registered */
  /* DKIM key records (zke_decode_key_records, zke_select_keys_from_records): helpers/src/dkim.rs:67-111 / RFC 6376 3.6.1.
   * zke_key_info.code: why a record yields no key.  100..109 */
  ZKE_D_KEYREC_NO_KEY        = 100, /* no p= in the record, the record ends with "p=", p= is empty (revoked), or the record is empty
                                       (the fetch failed)                                              dkim.rs:69-72, :92-94 */
  ZKE_D_KEYREC_B64           = 101, /* p= is not padded base64 STANDARD with zero trailing bits       dkim.rs:97, :104 */
  ZKE_D_KEYREC_TYPE          = 102, /* k= is neither "rsa" nor "ed25519" ("Unsupported key type")     dkim.rs:110 */
  ZKE_D_KEYREC_DER           = 103, /* k=rsa: neither a DER SubjectPublicKeyInfo (rsaEncryption, NULL parameter, 0 unused bits)
                                       nor a DER PKCS#1 RSAPublicKey                                   dkim.rs:98-99 */
  ZKE_D_KEYREC_RANGE         = 104, /* k=rsa: modulus > 4096 bits, e < 2 or e > 2^33-1 (as ZKE_D_KEY_RANGE) */
  ZKE_D_KEYREC_ED25519_LEN   = 105, /* k=ed25519: the decoded key is not 32 bytes                     dkim.rs:105-107 */
  ZKE_D_KEYREC_VERSION       = 106, /* ZKE_KEYREC_DNS: v= is not the first tag, or is not "DKIM1" */
  ZKE_D_KEYREC_SYNTAX        = 107, /* ZKE_KEYREC_DNS: the record is no tag-list, or holds a byte >= 0x80 */
  ZKE_D_KEYREC_NON_ASCII_EDGE = 108, /* ZKE_KEYREC_ARCHIVE: a ';'-separated part begins or ends, after ASCII trimming, with a byte
                                       >= 0x80: str::trim trims Unicode white space there, the engine trims ASCII only.  "Cannot
                                       answer", never a guess */
  ZKE_D_KEYREC_TOO_LONG      = 109, /* the record is longer than ZKE_KEYREC_MAX_BYTES */
  /* body extraction (zke_extract_bodies): the rule of strict RFC 4648 base64 a body breaks (ZKE_BODY_DECODE_FAIL), named so that a
   * more permissive decoder in the real crate shows up as a named difference; and the transfer encoding that is not decided */
  ZKE_D_BODY_B64_CHAR        = 110, /* after the ASCII white space is dropped: a byte outside the alphabet, or '=' anywhere but in the last two places */
  ZKE_D_BODY_B64_LENGTH      = 111, /* ... the length is no multiple of 4 (padding is required) */
  ZKE_D_BODY_B64_TRAILING_BITS = 112, /* ... the bits of the last character that belong to no byte are not zero */
  ZKE_D_U_BODY_CTE           = 113  /* ZKE_UNSUPPORTED: the chosen part's Content-Transfer-Encoding value holds bytes >= 0x80 or an RFC 2047 encoded word */
};
#define ZKE_D_DFA_BWD_OFFSET 10u /* added to ZKE_D_DFA_LABEL .. ZKE_D_DFA_QUITSET when the reverse blob is the one that fails (80..88) */

#define ZKE_MAX_HEADERS 256u   /* header fields per email the device parser tables hold */
#define ZKE_MAX_TAGS    32u    /* tag-specs per DKIM-Signature */
#define ZKE_MAX_TAGBUF  2048u  /* bytes of FWS-stripped tag values per DKIM-Signature */
#define ZKE_MAX_RSA_BYTES 512u /* RSA-4096, the rsa crate's ceiling (rsa 0.9.6 RsaPublicKey::MAX_SIZE) */
#define ZKE_CAP_MAX_STATES 8192u        /* states of a capture program (zke_capture_register) */
#define ZKE_CAP_MAX_PROGRAM_GROUPS 32u  /* groups of a capture program, group 0 included */
#define ZKE_CAP_MAX_GROUPS 16u          /* groups requested per part (zke_capture_part.n_groups) */
#define ZKE_CAP_MAX_SPAN   4096u        /* bytes of a match whose groups are extracted */
#define ZKE_CAP_MAX_PARTS  16u          /* parts of one extraction batch */
#define ZKE_CAPF_NOT_UTF8  1u           /* zke_capture_out.flags: the group's bytes are not valid UTF-8 (the host applies from_utf8_lossy) */
#define ZKE_KEY_RSA 0u
#define ZKE_KEY_ED25519 1u
#define ZKE_KEY_OTHER 2u

/* flags in zke_result.flags */
#define ZKE_F_HDR_RELAXED  1u
#define ZKE_F_BODY_RELAXED 2u
#define ZKE_F_HAS_LENGTH   4u
#define ZKE_F_SHA1         8u   /* a=rsa-sha1: body_hash / header_hash hold 20-byte SHA-1 digests, zero padded */
#define ZKE_F_ED25519      16u  /* a=ed25519-sha256 with an Ed25519 key (RFC 8463): Ed25519 over the SHA-256 header hash */

/* ------------------------------------------------------------------ result record */
/* Fixed 192-byte record per email.  from_domain_hash / public_key_hash are the
 * EmailVerifierOutput witnesses (core/src/circuits.rs:16-17); body_hash, header_hash,
 * lengths and the match span are intermediates exposed so parity is checkable
 * (SURVEY.md §0 item 5). external_inputs / regex_matches are echoes of the inputs
 * (circuits.rs:18-27, regex.rs:47) and are reassembled by the host wrapper. */
typedef struct zke_result {
  uint32_t status;            /* ZKE_* */
  uint32_t detail;            /* ZKE_D_* */
  uint32_t sig_index;         /* index among DKIM-Signature headers (file order) that passed / was tried last */
  uint32_t flags;             /* ZKE_F_* of that signature */
  uint32_t canon_header_len;  /* bytes in the header-hash preimage */
  uint32_t canon_body_len;    /* bytes hashed for bh (after l=) */
  uint32_t body_offset;       /* offset of the body in raw_email (first CRLFCRLF + 4) */
  uint32_t n_headers;         /* header fields mailparse would return */
  uint8_t  from_domain_hash[32];
  uint8_t  public_key_hash[32];
  uint8_t  body_hash[32];     /* SHA-256(canon body[..l]) of the signature in sig_index */
  uint8_t  header_hash[32];   /* SHA-256(header preimage) */
  uint32_t regex_part;        /* part index (header parts first, then body parts) checked last; 0xFFFFFFFF if none */
  uint32_t match_count;       /* matches found in that part, saturating at 2 */
  uint32_t match_start;       /* span of its first match */
  uint32_t match_end;
  uint32_t rsa_bits;          /* modulus bit length */
  uint32_t reserved[3];
} zke_result;

/* ------------------------------------------------------------------ batch input */
/* Struct-of-arrays view of &[Email] / &[EmailWithRegex] (core/src/structs.rs:49-62).
 * Caller-owned, read-only for the call.  In zke_verify_batch / zke_verify_batch_async the
 * pointers are host memory and every offset array is checked to be non-decreasing before
 * anything is copied (ZKE_E_ARG otherwise); in zke_verify_batch_device they are device (HBM)
 * pointers and the offsets are trusted like the pointers themselves. */
typedef struct zke_batch {
  uint32_t n;                      /* emails */
  const uint8_t*  raw_blob;        /* Email.raw_email, concatenated            structs.rs:51 */
  const uint64_t* raw_off;         /* [n+1] */
  const uint8_t*  domain_blob;     /* Email.from_domain (UTF-8)                structs.rs:50 */
  const uint64_t* domain_off;      /* [n+1] */
  const uint8_t*  key_blob;        /* Email.public_key.key (PKCS#1 DER for rsa) structs.rs:9 */
  const uint64_t* key_off;         /* [n+1] */
  const uint8_t*  key_type;        /* [n] ZKE_KEY_*  (PublicKey.key_type)      structs.rs:10 */
  const uint8_t*  ext_null;        /* [n] or NULL: 1 if any ExternalInput.value is None (circuits.rs:24) */

  /* regex section (EmailWithRegex.regex_info, structs.rs:32-35,59-62).  The part list
   * is shared by the batch (one regex_config per batch); captures are per email. */
  uint32_t with_regex;             /* 0: verify_email; 1: verify_email_with_regex */
  uint32_t n_header_parts;
  uint32_t n_body_parts;
  const uint32_t* header_part_ids; /* [n_header_parts] ids from zke_dfa_register */
  const uint32_t* body_part_ids;   /* [n_body_parts] */
  /* captures of email i, part p (p over header parts then body parts, P = total):
   * strings cap_str_off[ cap_off[i*P+p] .. cap_off[i*P+p+1] ) in cap_blob. */
  const uint32_t* cap_off;         /* [n*P + 1], or NULL: no captures.  cap_off[n*P] == 0 (no string anywhere) is the same as
                                      NULL, and cap_str_off / cap_blob may then be NULL; otherwise both are required */
  const uint32_t* cap_str_off;     /* [n_strings + 1] */
  const uint8_t*  cap_blob;
} zke_batch;

/* Optional copies of the intermediates, for parity tests (host mode only).  Any
 * pointer may be NULL.  Slot i of a blob starts at i*stride. */
typedef struct zke_debug_out {
  uint8_t* canon_header; size_t canon_header_stride;  /* header-hash preimage */
  uint8_t* canon_body;   size_t canon_body_stride;    /* canonicalised body (before l=) */
  uint8_t* clean_body;   size_t clean_body_stride;    /* after remove_quoted_printable_soft_breaks (email.rs:61-86) */
  uint8_t* em;           size_t em_stride;            /* sig^e mod n, big-endian, k bytes */
  uint32_t* canon_body_full_len;                      /* [n] canonical body length before l= */
  uint32_t* rsa_route;                                /* [n] which RSA routine takes the e-mail's signatures: 4 four lanes per signature,
                                                         8 eight lanes (the key's constants were cached); else one signature per
                                                         wave and why: 0x100 no lane-group kernel for this size in the launch,
                                                         0x200 key not cached yet, 0x400 cache slot taken, 0x800 not eligible */
} zke_debug_out;

/* Engine options.  A zero-filled struct (or NULL) is the default configuration: every field is phrased so that 0 means
 * "what the engine does by default".  ABI 0.3: the fields have names (0.2 kept them in reserved[]). */
typedef struct zke_options {
  int32_t  device;              /* HIP device ordinal; -1 = the calling thread's current device.  NOTE: 0 is device 0. */
  uint32_t slots;               /* submission slots created with the engine (0 = 1); zke_engine_reserve can raise it later */
  uint32_t max_sig_rounds;      /* same-domain DKIM-Signature headers tried per e-mail, in file order, until one passes — cfdkim
                                   tries them all; 0 = 16, at most ZKE_MAX_HEADERS.  The first is tried in the batch's three
                                   launches, later ones inside the last of them by the e-mail's own wave.  An e-mail with more
                                   failing candidates reports ZKE_UNSUPPORTED / ZKE_D_U_TOO_MANY_SIGS. */
  uint32_t disable_key_cache;   /* 1: no per-key Montgomery-constant cache (R^2 mod n recomputed per signature) */
  uint32_t host_threads;        /* worker threads that copy host-entry batches into pinned staging memory (0 = 4; 1 = the caller's
                                   thread alone).  zke_verify_batch[_async] only. */
  uint32_t max_dfas;            /* DFA pairs the registry holds before it evicts pairs that zke_verify_email_with_regex registered
                                   on its own (0 = 4096) */
  /* kernel variants (0 = chosen by batch size; the parity tests force each; sha_mapping below is one more) */
  uint32_t rsa_lane_groups;     /* 1: never the four- / eight-lanes-per-signature RSA routines; 2: always */
  uint32_t dfa_mapping;         /* 1: one e-mail per lane for every regex part; 2: one e-mail per wave for every part */
  uint32_t replay_graphs;       /* 1: zke_verify_batch_device replays a captured hipGraph when a slot sees the same descriptor
                                   again (measured slower than plain launches on MI355X: DESIGN.md §5) */
  /* Strictness flags: behaviours of the reference's un-vendored crates that could not be verified offline (SURVEY.md
   * Appendix B "open questions").  0 = this engine's reading of cfdkim@75af99fb; 1 = the other reading.  Each
   * flag switches ONE named site in the device front end (csrc/parse.hip.h, ZKE_STRICT_*) and the same site in the CPU
   * oracle (oracle/zke_oracle.c), so a maintainer with the Rust crates at hand flips a field, not a kernel. */
  uint32_t enforce_expiry_x;             /* 1: a signature whose x= tag lies before `now_unix` fails (ZKE_D_SIG_EXPIRED), as
                                            cloudflare/dkim's validate_header does; 0: x= is ignored (a zkVM guest has no clock) */
  uint32_t canon_takes_verified_signature; /* canonicalize_signed_email (core/src/circuits.rs:34-35) — 0: the FIRST DKIM-Signature
                                            header of the e-mail, whatever its d=; 1: the signature verify_dkim accepted */
  uint32_t canon_ignores_l;              /* 0: canonicalize_signed_email truncates the canonical body to l=, as the verify path
                                            does; 1: it returns the whole canonical body */
  uint32_t i_must_be_subdomain;          /* i= check — 0: i= ends with d= (a plain suffix test); 1: the domain of i= (behind its
                                            last '@') equals d= or ends with "." d=, case-insensitively (RFC 6376 §3.5) */
  uint32_t b_removes_own_span_only;      /* 0: the raw b= value is removed wherever it occurs in the header (String::replace);
                                            1: only the b= tag's own span is emptied */
  /* one more kernel variant, as rsa_lane_groups / dfa_mapping above (0 = chosen by launch size; the parity tests force each) */
  uint32_t sha_mapping;         /* hash stage — 1: always one wave per 64 messages (for a batch: a hash launch of its own, then the
                                   RSA roles); 2: always two waves per 64 messages (for a batch: fused with the RSA roles) */
  uint64_t now_unix;            /* the time x= is compared with (enforce_expiry_x); 0 = the host clock at submission */
  uint64_t reserved[4];         /* 0 */
} zke_options;

/* bits of the strictness mask the kernels and the oracle take (one per flag above, same order) */
#define ZKE_STRICT_EXPIRY_X        1u
#define ZKE_STRICT_CANON_VERIFIED  2u
#define ZKE_STRICT_CANON_IGNORES_L 4u
#define ZKE_STRICT_I_SUBDOMAIN     8u
#define ZKE_STRICT_B_OWN_SPAN      16u

typedef struct zke_engine zke_engine;

/* Device time of one batch's launches, microseconds (HIP events on the stream the batch ran on; zke_set_timing). */
typedef struct zke_timings {
  float front_end_us;     /* parse_kernel: header split, key decode, tag lists, header-hash preimage, body canonicalisation */
  float hash_modexp_us;   /* hash_modexp_kernel: the SHA-256 groups beside the RSA roles (one launch) */
  float ed_verdict_us;    /* ed_verdict_kernel: Ed25519 stage, verdicts, later signature rounds */
  float regex_prep_us;    /* verify_email_with_regex: canonicalize_signed_email pass + QP soft-break removal */
  float dfa_us;           /* ... the DFA launches and the regex verdict */
  float total_us;         /* first launch to last launch (copies excluded) */
  float h2d_us, d2h_us;   /* host entry only: the packed input image in, the records out */
} zke_timings;

/* All functions return 0 on success, or a negative code if the CALL failed (bad
 * arguments, device error, extension missing).  They never abort on a bad email. */
#define ZKE_E_ARG     (-1)
#define ZKE_E_DEVICE  (-2)
#define ZKE_E_NOMEM   (-3)
#define ZKE_E_DFA     (-4)

/* Process-wide set-up, optional.  HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and reads the
 * variable once, when the runtime initialises; every submission slot wants a queue of its own, and MI355X runs 24 queues of a
 * process without time-slicing them.  zke_process_init(q) exports GPU_MAX_HW_QUEUES = q (0 = 23: 22 slots + the
 * null stream) unless the variable is already set.  It has an effect only before the process's first HIP call: call it first
 * thing in main().  zke_engine_create calls zke_process_init(0) itself, which covers hosts whose first HIP call is that
 * one; a host that has used HIP before (a framework, another library) keeps the pool it has and should call this itself,
 * earlier.  Nothing else in this library touches the process environment, and nothing runs at load time. */
int zke_process_init(uint32_t hw_queues);

int zke_engine_create(const zke_options* opt, zke_engine** out);
/* Waits for everything in flight — batches submitted on a caller's stream included — before it frees anything; host batches
 * nobody waited for are delivered to their `out` arrays on the way out.  (Building-block launches on a caller's stream,
 * zke_sha256_batch_device, are not tracked: the caller synchronises them first.) */
void zke_engine_destroy(zke_engine* e);
/* The message of the last failed call on this engine by the calling thread ("" if none). */
const char* zke_last_error(const zke_engine* e);

/* Threading.  The reference's two functions are re-entrant (core/src/circuits.rs:9: no state between calls), and so are
 * the entry points here: zke_verify_batch, zke_verify_batch_async / zke_batch_wait, zke_verify_batch_device,
 * zke_verify_email, zke_verify_email_with_regex and zke_dfa_register may be called from any number of host threads on ONE
 * engine at once.  Each call takes the next submission slot (an atomic ticket) and holds that slot's lock while it
 * enqueues; everything a call needs lives in its slot.  zke_engine_reserve, zke_dfa_unregister and zke_engine_destroy
 * are exclusive: they wait for the submissions in progress and hold new ones off. */

/* One engine per GPU.  An engine owns `slots` submission slots — a stream, a private workspace and (host entry) a pinned
 * staging image each — so that many batches can be in flight at once; what batches share (the per-key Montgomery constants
 * of the RSA kernels, the registered DFA tables, kernel attributes) exists once per engine.
 * zke_engine_reserve(e, max_n, max_raw_total, slots, max_regex_parts) raises the slot count to `slots` (1..64) and sizes
 * every slot's workspace for batches of up to max_n e-mails / max_raw_total raw bytes (max_regex_parts > 0: the
 * verify_email_with_regex buffers too), so that no allocation happens in the submit path afterwards.  A larger batch
 * still works: its slot grows (one synchronising reallocation).
 * With max_regex_parts > 0 every slot also gets the buffers of a capture extraction (zke_extract_captures), whether or not the
 * caller ever extracts: the spans, flags and tables of max_n e-mails with FOUR requested groups per part and 32 bytes of blob per
 * group, their pinned twin (host memory), and 34.6 MB of HBM for the reachability rows of capture programs with more than 512
 * states.  An extraction with more groups per part, or whose caller passes a larger cap_blob, regrows its slot's buffers on first
 * use (one synchronising reallocation), as a larger batch does. */
int zke_engine_reserve(zke_engine* e, uint32_t max_n, uint64_t max_raw_total, uint32_t slots, uint32_t max_regex_parts);
/* The same for the host entry's staging: every slot's pinned input image and record buffer (and their HBM twins) are sized
 * for batches of up to max_n e-mails whose inputs — raw e-mails + from_domains + keys (+ captures) — total max_input_bytes.
 * Pinned memory is a host resource (S slots x image bytes): a caller that only uses zke_verify_batch_device never pays it,
 * and without this call a slot's staging comes into being with its first host batch. */
int zke_engine_reserve_host(zke_engine* e, uint32_t max_n, uint64_t max_input_bytes);

/* Parse one regex-automata 0.4 dense-DFA pair once (replaces the per-email
 * dense::DFA::from_bytes of core/src/regex.rs:32-33), validate it and stage a repacked
 * transition table on the device.  Accepts unaligned input, so the align_slice shim
 * (core/src/regex.rs:5-13) is unnecessary.  A blob that from_bytes would reject still
 * gets an id; emails using it report ZKE_DFA_DECODE_FAIL with the failing section as `detail` (ZKE_D_DFA_*).
 * An equal pair registered again gets its old id (the registry is keyed by a hash of the pair). */
int zke_dfa_register(zke_engine* e, const uint8_t* fwd, size_t fwd_len,
                     const uint8_t* bwd, size_t bwd_len, uint32_t* out_id);
/* *detail = 0 when both blobs of pair `id` deserialise, else the ZKE_D_DFA_* section at which from_bytes gives up. */
int zke_dfa_status(zke_engine* e, uint32_t id, uint32_t* detail);
/* Drop a registered pair and free its tables (waits for the batches in flight).  The id may be given out again. */
int zke_dfa_unregister(zke_engine* e, uint32_t id);

/* Host-memory batch — what a drop-in caller has: `&[Email]` in RAM (core/src/circuits.rs:9 takes a host-resident &Email,
 * built at helpers/src/generator.rs:40-45).  The offsets, key types and the three blobs are packed into ONE image in the
 * slot's pinned staging buffer (by `host_threads` workers for large batches), cross PCIe as ONE copy on the slot's
 * stream, the three launches follow, and the n records come back as one copy into pinned memory.
 *   zke_verify_batch_async  returns as soon as everything is enqueued; `in` has been read completely (the caller may reuse
 *                           its buffers), `out` must stay valid until zke_batch_wait(e, *ticket) has returned.  With S slots
 *                           reserved, S batches are in flight; a slot whose previous batch was never waited for completes it
 *                           (its records are delivered) before it is reused, and at the latest when S further batches have
 *                           been submitted (slots on a fuller hardware queue come round later than that: zke_engine_slot_queue).
 *   zke_batch_wait          blocks until that batch's records are in `out`.  Waiting twice, or for a ticket a later batch of
 *                           the same slot has already retired, returns 0 at once.
 *   zke_verify_batch        = async + wait; `dbg` != NULL additionally copies the parity intermediates back (tests). */
int zke_verify_batch(zke_engine* e, const zke_batch* in, zke_result* out, zke_debug_out* dbg);
int zke_verify_batch_async(zke_engine* e, const zke_batch* in, zke_result* out, uint64_t* ticket);
int zke_batch_wait(zke_engine* e, uint64_t ticket);

/* The reference's own layout: n separate Email values, each with buffers of its own (`&[Email]`: a Vec<u8> and two Strings per
 * e-mail, core/src/structs.rs:49-54) instead of three concatenated blobs.  The engine gathers them straight into its pinned
 * staging image on its packing threads — ONE copy between the caller's Vecs and the DMA engine — and computes the CSR offsets
 * itself; a caller that would only concatenate the buffers to call zke_verify_batch saves that pass (a single-threaded copy of
 * the whole batch).  Same pipeline, same records, same ticket protocol as zke_verify_batch_async; verify_email only (regex
 * batches carry per-e-mail capture tables: zke_batch). */
typedef struct zke_email_ref {
  const uint8_t* raw;         size_t raw_len;        /* Email.raw_email */
  const char*    from_domain; size_t domain_len;     /* Email.from_domain (UTF-8, no terminator needed) */
  const uint8_t* key;         size_t key_len;        /* Email.public_key.key */
  uint32_t key_type;                                 /* ZKE_KEY_* of Email.public_key.key_type */
  uint32_t external_input_null;                      /* != 0: some ExternalInput.value is None (circuits.rs:24) */
} zke_email_ref;
int zke_verify_emails(zke_engine* e, const zke_email_ref* emails, uint32_t n, zke_result* out);
int zke_verify_emails_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, zke_result* out, uint64_t* ticket);
/* ... and verify_email_with_regex over `&[EmailWithRegex]` that share one part list (one regex_config per batch): the e-mails as
 * above, the part lists and the per-e-mail capture tables exactly as zke_batch has them (host arrays; small).  A slice that mixes
 * part lists: zke_verify_emails_mixed below. */
typedef struct zke_regex_lists {
  uint32_t n_header_parts; const uint32_t* header_part_ids;   /* ids from zke_dfa_register, RegexInfo.header_parts order */
  uint32_t n_body_parts;   const uint32_t* body_part_ids;
  const uint32_t* cap_off;         /* [n*P + 1] or NULL: no captures anywhere (as zke_batch.cap_off) */
  const uint32_t* cap_str_off;     /* [n_strings + 1] */
  const uint8_t*  cap_blob;
} zke_regex_lists;
int zke_verify_emails_with_regex(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_lists* lists, zke_result* out);
int zke_verify_emails_with_regex_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_lists* lists,
                                       zke_result* out, uint64_t* ticket);

/* ... and over `&[EmailWithRegex]` as the reference has it: every value carries its own RegexInfo (core/src/structs.rs:32-35,59-62;
 * core/src/circuits.rs:31-68 takes one at a time), so one batch may mix regex configs — a relayer's queue of receipts, invitations
 * and password resets, each with its own regex_config.json — and e-mails that are verify_email only.  `configs` are the distinct
 * part lists, config_of[i] names e-mail i's.  out[i] is exactly the record zke_verify_emails_with_regex gives e-mail i in a batch
 * that holds only its own config — status, detail, regex_part, match_*, the fold order "header parts, then body parts, stop at the
 * first failing part" — and for config_of[i] == ZKE_CONFIG_NONE the record of zke_verify_emails (circuits.rs:9): the regex stage
 * neither reads nor writes it.  A config with ZERO parts is not ZKE_CONFIG_NONE: it is verify_email_with_regex with both lists
 * None, which still runs canonicalize_signed_email(..).unwrap() (circuits.rs:34-35) and can report that failure.
 * On the device: the verify launches, one preparation launch, ONE lane-mapped and ONE wave-mapped DFA launch whatever the number of
 * configs and parts (a block is told by a segment table which config's e-mails and which automaton it owns), one verdict launch.
 * ZKE_E_ARG, before anything is staged: a config_of[i] that is neither below n_configs nor ZKE_CONFIG_NONE, n_configs above
 * ZKE_MIXED_MAX_CONFIGS, more than ZKE_MIXED_MAX_PARTS parts in a config, a null list with a non-zero count, capture offsets that
 * decrease.  An unknown or undecodable DFA id stays a per-e-mail matter: the e-mails of the configs that use it report
 * ZKE_DFA_DECODE_FAIL with the section.  Same slots, tickets and zke_batch_wait as zke_verify_emails_async; everything `mixed`
 * points to has been read when the call returns. */
#define ZKE_MIXED_MAX_CONFIGS 64u
#define ZKE_MIXED_MAX_PARTS 64u
#define ZKE_CONFIG_NONE 4294967295u
typedef struct zke_regex_config {     /* one RegexInfo's part lists */
  uint32_t n_header_parts; const uint32_t* header_part_ids;   /* ids from zke_dfa_register, RegexInfo.header_parts order */
  uint32_t n_body_parts;   const uint32_t* body_part_ids;
} zke_regex_config;
typedef struct zke_regex_mixed {
  uint32_t n_configs; const zke_regex_config* configs;
  const uint32_t* config_of;       /* [n]: index into configs, or ZKE_CONFIG_NONE: this e-mail is verify_email only */
  const uint32_t* cap_off;         /* [J + 1] or NULL: no captures anywhere.  J = the sum over the e-mails of P(config_of[i]) (0 for
                                      ZKE_CONFIG_NONE), e-mail-major: e-mail i's part p is job job_off[i] + p, header parts first,
                                      job_off the prefix sum of P; the captures of job j are the strings cap_off[j] .. cap_off[j + 1] */
  const uint32_t* cap_str_off;     /* [n_strings + 1], as zke_regex_lists */
  const uint8_t*  cap_blob;
} zke_regex_mixed;
int zke_verify_emails_mixed(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_mixed* mixed, zke_result* out);
int zke_verify_emails_mixed_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_regex_mixed* mixed,
                                  zke_result* out, uint64_t* ticket);

/* ---- capture extraction: the compute half of the reference's input generation (helpers/src/generator.rs:55-87 ->
 * helpers/src/regex.rs:16-51) — canonicalise, remove the QP soft breaks, require exactly one match per pattern, run the capturing
 * automaton over the match and turn the groups named by capture_indices into strings.  The DNS key fetch and the file IO stay with
 * the caller.  A capture program is the pattern's Thompson NFA with its capture states (zkemail_rs_amd.regex_compile.
 * create_capture_program; layout: DESIGN.md §3), registered once like a DFA pair: validated on the host — every state index, slot
 * and range — before a table reaches the device, de-duplicated by content.  A program that does not decode, or exceeds
 * ZKE_CAP_MAX_STATES / ZKE_CAP_MAX_PROGRAM_GROUPS, still gets an id; zke_capture_status says which (0, ZKE_D_U_CAPTURE_PROGRAM,
 * ZKE_D_U_CAPTURE_STATES) and e-mails that use it report ZKE_UNSUPPORTED with that detail. */
int zke_capture_register(zke_engine* e, const uint8_t* prog, size_t len, uint32_t* out_id);
int zke_capture_status(zke_engine* e, uint32_t id, uint32_t* detail);
int zke_capture_unregister(zke_engine* e, uint32_t id);      /* waits for the batches in flight */
/* The same check without an engine or a GPU (pure host code): *detail as zke_capture_status reports it. */
int zke_capture_validate(const uint8_t* prog, size_t len, uint32_t* detail);

typedef struct zke_capture_part {
  uint32_t dfa_id;                 /* from zke_dfa_register: finds the match */
  uint32_t prog_id;                /* from zke_capture_register: the same pattern's capture program */
  uint32_t n_groups;               /* <= ZKE_CAP_MAX_GROUPS */
  const uint32_t* groups;          /* [n_groups] RegexPattern.capture_indices (group 0 = the whole match) */
} zke_capture_part;

/* Where the extraction goes: caller-sized buffers, the sizes needed written back (the zke_abi_encode convention).  With G = the
 * sum of n_groups over the parts and P parts: spans, flags, cap_off and cap_str_off have sizes known up front — n*G*2, n*G, n*P+1
 * and n*G+1 entries; a call whose buffers are smaller fails at once with ZKE_E_NOMEM and the *_need fields set.  cap_blob's size
 * depends on the e-mails: when it is too small the call (zke_batch_wait for the asynchronous form) returns ZKE_E_NOMEM, records,
 * spans, flags and both offset tables are delivered all the same, and cap_blob_need says what a second call needs (a group's bytes
 * never exceed its match span, so n * G * ZKE_CAP_MAX_SPAN always suffices).  String offsets are 32-bit as in zke_batch: a call with
 * n * G * ZKE_CAP_MAX_SPAN >= 4 GiB (n * G >= 2^20) is refused with ZKE_E_ARG — split the batch.
 *   spans  {start, end} per (e-mail, requested group), relative to the part's haystack — the canonical header for header parts,
 *          the QP-cleaned canonical body for body parts; {0xFFFFFFFF, 0xFFFFFFFF}: no string (the e-mail failed)
 *   flags  ZKE_CAPF_* per (e-mail, requested group)
 *   cap_off / cap_str_off / cap_blob   the capture tables exactly as zke_batch / zke_regex_lists take them: raw bytes, no UTF-8
 *          repair.  An e-mail whose record is not ZKE_OK has no strings. */
typedef struct zke_capture_out {
  uint32_t* spans;       size_t spans_cap;         /* capacities in ENTRIES of the array's type */
  uint8_t*  flags;       size_t flags_cap;
  uint32_t* cap_off;     size_t cap_off_cap;
  uint32_t* cap_str_off; size_t cap_str_off_cap;
  uint8_t*  cap_blob;    size_t cap_blob_cap;
  size_t spans_need, flags_need, cap_off_need, cap_str_off_need, cap_blob_need;     /* written by the call */
  size_t n_strings;                                                                 /* entries of cap_str_off in use, minus one */
} zke_capture_out;

/* verify_email + the extraction over n e-mails that share one part list, on the gathering host entry (same slots, tickets and
 * zke_batch_wait as zke_verify_emails_async).  Records: DKIM failure -> its usual status; match count != 1 -> ZKE_HEADER_REGEX_FAIL
 * / ZKE_BODY_REGEX_FAIL + ZKE_D_RE_MATCH_COUNT ("Input doesn't match regex pattern"); a requested group absent or not taking part
 * -> the same statuses + ZKE_D_RE_GROUP_MISSING; over a limit -> ZKE_UNSUPPORTED + ZKE_D_U_CAPTURE_*.  ONE fold, as
 * compile_regex_parts walks the parts (helpers/src/regex.rs:21-47: a part's match count, then its groups, then the next part): the
 * record names the first part in verify order (header parts, then body parts) that fails for any reason — a missing group in part 0
 * is reported in front of a wrong match count in part 1; regex_part, match_count, match_start, match_end keep their meaning and
 * are those of the part named.  At most ZKE_CAP_MAX_PARTS parts per call (ZKE_E_ARG beyond).  `caps` (and what it points to) must stay valid until the batch has been waited for. */
int zke_extract_captures(zke_engine* e, const zke_email_ref* emails, uint32_t n,
                         const zke_capture_part* header_parts, uint32_t n_header_parts,
                         const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out, zke_capture_out* caps);
int zke_extract_captures_async(zke_engine* e, const zke_email_ref* emails, uint32_t n,
                               const zke_capture_part* header_parts, uint32_t n_header_parts,
                               const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out, zke_capture_out* caps,
                               uint64_t* ticket);
/* Building block: one part over n plain host haystacks hay_blob[hay_off[i] .. hay_off[i+1]) — find the match (exactly one, as
 * core/src/regex.rs:37 counts), extract the groups.  matches[4*i ..] = {code, count, start, end}: code 0, or the ZKE_D_* that
 * fails the haystack (ZKE_D_RE_MATCH_COUNT, ZKE_D_RE_QUIT, ZKE_D_RE_GROUP_MISSING, ZKE_D_U_CAPTURE_*; an undecodable DFA pair:
 * its ZKE_D_DFA_* section).  `caps` as above with P = 1, G = n_groups. */
int zke_capture_batch(zke_engine* e, uint32_t dfa_id, uint32_t prog_id, const uint32_t* groups, uint32_t n_groups,
                      const uint8_t* hay_blob, const uint64_t* hay_off, uint32_t n, uint32_t* matches, zke_capture_out* caps);

/* ---- the index map of remove_quoted_printable_soft_breaks (core/src/email.rs:61-86): the function returns (cleaned, index_map),
 * verify_email_with_regex discards the map (circuits.rs:37), a proving flow cannot — an extraction reports its spans in the
 * QP-cleaned body, a circuit or a zkVM guest is given the body as it was signed (the canonical body, whose hash is bh=).
 * Building block: the reference function over n plain host bodies body_blob[body_off[i] .. body_off[i+1]), both return values.
 * cleaned (body_off[n] - body_off[0] bytes) and index_map (as many entries) are laid out by the same offsets, rebased to
 * body_off[0]: cleaned is the reference's first value, zero-padded to the body's length; index_map[j] is the position within its
 * body of cleaned byte j, ZKE_QP_NO_INDEX (the reference's usize::MAX in this ABI's 32-bit positions) from clean_len[i] on;
 * clean_len[i] is the number of bytes kept.  Any of the three outputs may be NULL, not all of them (ZKE_E_ARG).  Offsets must
 * be non-decreasing and a body shorter than 2^32 - 1 bytes (ZKE_E_ARG).  Synchronous; runs in one slot, in buffers that only grow. */
#define ZKE_QP_NO_INDEX 4294967295u
int zke_qp_clean_batch(zke_engine* e, const uint8_t* body_blob, const uint64_t* body_off, uint32_t n,
                       uint8_t* cleaned, uint32_t* index_map, uint32_t* clean_len);

/* ---- String::from_utf8_lossy (helpers/src/regex.rs:35): the step between the bytes a capture group matched and the string the
 * reference keeps in CompiledRegex.captures.  The rule is core::str::Utf8Chunks': every maximal prefix of a well-formed sequence
 * (Unicode Table 3-7) that is not itself well-formed becomes one U+FFFD (EF BF BD), and so does every byte no sequence covers — a
 * stray continuation byte, C0, C1, F5..FF — and a sequence cut short by the end of the string; well-formed bytes are copied
 * (61 F1 80 80 E1 80 C2 62 80 63 80 BF 64 -> 61 FFFD FFFD FFFD 62 FFFD 63 FFFD FFFD 64).
 * Building block: the function over n plain host strings blob[off[i] .. off[i+1]).  out_off[n + 1] is the CSR of the repaired
 * strings (out_off[0] = 0), flags[i] bit 0 says string i was changed (it was not valid UTF-8), out_blob takes the repaired bytes:
 * *out_blob_need is always written; when out_blob_cap is smaller the call returns ZKE_E_NOMEM, out_off and flags are delivered all
 * the same, nothing is written into out_blob and a second call with *out_blob_need bytes suffices (three times the input always
 * does).  The repaired offsets are 32-bit: strings of more than ZKE_UTF8_LOSSY_MAX_BYTES bytes in all, or offsets that decrease,
 * are refused with ZKE_E_ARG before anything is staged.  Synchronous; runs in one slot, in buffers that only grow. */
#define ZKE_UTF8_LOSSY_MAX_BYTES 1431655765u   /* (2^32 - 1) / 3 */
int zke_utf8_lossy_batch(zke_engine* e, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t* out_off, uint8_t* out_blob,
                         size_t out_blob_cap, size_t* out_blob_need, uint8_t* flags);

/* zke_extract_captures that also says where each span lies BEFORE the QP filter.  Records, caps, statuses and the one fold are
 * those of zke_extract_captures on the same input; `org` is filled in addition (sizes known up front, the zke_capture_out
 * convention: too small fails at once with ZKE_E_NOMEM and the *_need fields set).  With im = the index map of the e-mail's regex
 * haystack (its canonical body, n bytes: after l= unless ZKE_STRICT_CANON_IGNORES_L) and {s, e} the entry of caps.spans:
 *   header part, or an e-mail without strings ({0xFFFFFFFF, 0xFFFFFFFF})    origin = {s, e}, flags 0 (a header is never cleaned)
 *   body part    start = s < n ? im[s] : ZKE_QP_NO_INDEX
 *                end   = e == s ? start : (im[e-1] == ZKE_QP_NO_INDEX ? ZKE_QP_NO_INDEX : im[e-1] + 1)
 *                ZKE_ORGF_PADDING iff either member is ZKE_QP_NO_INDEX; else ZKE_ORGF_SPLIT iff end - start != e - s
 * With no flag set, canonical_body[start:end] equals the capture's bytes. */
#define ZKE_ORGF_SPLIT   1u  /* a soft break was removed inside the span: end-start of the origin != end-start of the span */
#define ZKE_ORGF_PADDING 2u  /* the span reaches into the zero padding: a member of the origin is ZKE_QP_NO_INDEX */
typedef struct zke_capture_origin {
  uint32_t* spans; size_t spans_cap;   /* n*G*2: {start, end} in the haystack BEFORE the QP filter */
  uint8_t*  flags; size_t flags_cap;   /* n*G   ZKE_ORGF_* */
  size_t spans_need, flags_need;       /* written by the call */
} zke_capture_origin;
int zke_extract_captures_mapped(zke_engine* e, const zke_email_ref* emails, uint32_t n,
                                const zke_capture_part* header_parts, uint32_t n_header_parts,
                                const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out, zke_capture_out* caps,
                                zke_capture_origin* org);
int zke_extract_captures_mapped_async(zke_engine* e, const zke_email_ref* emails, uint32_t n,
                                      const zke_capture_part* header_parts, uint32_t n_header_parts,
                                      const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out, zke_capture_out* caps,
                                      zke_capture_origin* org, uint64_t* ticket);

/* The extraction over `&[Email]` whose e-mails carry DIFFERENT regex configs — what produces, in one call, the values
 * zke_verify_emails_mixed consumes: `configs` are the distinct RegexConfigs (parts with their programs and requested groups),
 * config_of[i] names e-mail i's, ZKE_CONFIG_NONE an e-mail that is verify_email only.
 * Layout.  With P_i and G_i the part count and the requested-group count of e-mail i's config (both 0 for ZKE_CONFIG_NONE), job_off
 * and col_off their prefix sums, J = job_off[n] and Gt = col_off[n]: part p of e-mail i is job job_off[i] + p, header parts first,
 * exactly as in zke_regex_mixed; requested group k of that part is column col_off[i] + gbase[p] + k, gbase the prefix sum of the
 * config's per-part group counts.  `caps` sizes are known up front — spans 2*Gt, flags Gt, cap_off J+1, cap_str_off Gt+1 — and so
 * are `org`'s (NULL: no origins): spans 2*Gt, flags Gt.  Both follow the conventions of zke_capture_out / zke_capture_origin: too
 * small fails at once with ZKE_E_NOMEM and the *_need fields set; a short cap_blob delivers everything else and reports
 * cap_blob_need exactly.  cap_off / cap_str_off / cap_blob are byte for byte what zke_regex_mixed takes.
 * Records.  out[i], the e-mail's spans, flags, strings and origins are exactly what zke_extract_captures[_mapped] gives e-mail i in a
 * batch that holds only its own config, the single fold included (the first failing part in verify order, for either reason).  For
 * ZKE_CONFIG_NONE out[i] is the record of zke_verify_emails: the e-mail has no job and no column, and the regex and capture stages
 * neither read nor write it.
 * ZKE_E_ARG, before anything is staged (`out` and `caps` untouched): n_configs above ZKE_MIXED_MAX_CONFIGS; a config with 0 parts or
 * more than ZKE_CAP_MAX_PARTS (the single-config entry's rule: ZKE_CONFIG_NONE is the way to say "no regex"); a part asking for more
 * than ZKE_CAP_MAX_GROUPS groups; a null list with a non-zero count; a config_of[i] that is neither below n_configs nor
 * ZKE_CONFIG_NONE; Gt * ZKE_CAP_MAX_SPAN >= 4 GiB (Gt >= 2^20).
 * An unknown or undecodable DFA or program id fails only the e-mails of the configs that use it: ZKE_DFA_DECODE_FAIL with the
 * section, or ZKE_UNSUPPORTED / ZKE_D_U_CAPTURE_*.  Slots, tickets, zke_batch_wait and the lifetimes of `caps` / `org` are as for
 * zke_extract_captures_async; everything `mixed` points to has been read when the call returns.  The slot's capture buffers are
 * sized by J and Gt and only grow; zke_engine_reserve's sizing is unchanged, so a mixed extraction larger than the reserved shape
 * (max_n * max_regex_parts jobs, four groups per part) regrows them once, as a larger batch does. */
typedef struct zke_capture_config {          /* one RegexConfig: the parts with their programs and requested groups */
  uint32_t n_header_parts; const zke_capture_part* header_parts;
  uint32_t n_body_parts;   const zke_capture_part* body_parts;
} zke_capture_config;
typedef struct zke_capture_mixed {
  uint32_t n_configs; const zke_capture_config* configs;
  const uint32_t* config_of;                 /* [n]: index into configs, or ZKE_CONFIG_NONE: verify_email only */
} zke_capture_mixed;
int zke_extract_captures_mixed(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_mixed* mixed, zke_result* out,
                               zke_capture_out* caps, zke_capture_origin* org /* NULL: no origins */);
int zke_extract_captures_mixed_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_capture_mixed* mixed, zke_result* out,
                                     zke_capture_out* caps, zke_capture_origin* org, uint64_t* ticket);

/* ---- DKIM-Signature scan and key selection: the compute on both sides of the caller's DNS fetch in the reference's
 * generate_email_inputs (helpers/src/generator.rs:11-53).  The fetch itself, like all IO, stays with the caller:
 *     zke_scan_signatures   raw e-mails + from_domain -> per e-mail every DKIM-Signature header with its validate_header verdict,
 *                           selector and algorithm                                                   (generator.rs:17-30)
 *     (the caller resolves selector._domainkey.domain for the candidates)                            (generator.rs:31-34)
 *     zke_select_keys       per e-mail the candidate keys in -> the first one under which verify_email passes, and that
 *                           verification's record                                                    (generator.rs:36-45)
 * Both go through the gathering host entry: same slots, tickets and zke_batch_wait as zke_verify_emails_async. */
#define ZKE_SCAN_MAX_SIGS 64u           /* records per e-mail a scan lists at most (its max_sigs argument: 1 .. this) */
#define ZKE_SIG_ALGO_RSA_SHA256     0u  /* zke_sig_info.algo: a= as the front end classifies it */
#define ZKE_SIG_ALGO_RSA_SHA1       1u
#define ZKE_SIG_ALGO_ED25519_SHA256 2u
#define ZKE_SIG_ALGO_OTHER          3u
#define ZKE_SEL_NONE              4294967295u /* 0xFFFFFFFF; zke_select_keys chosen[i]: no candidate key verifies the e-mail */
#define ZKE_SEL_AFTER_UNSUPPORTED 2147483648u /* 0x80000000; ... bit 31 beside an index: a candidate in front of the chosen one reported
                                                 ZKE_UNSUPPORTED and might have passed in the reference: reported, never guessed */

typedef struct zke_sig_info {      /* 32 bytes */
  uint32_t header_index;           /* index of the header field in the message */
  uint32_t code;                   /* 0 candidate | ZKE_D_NEUTRAL other domain | ZKE_D_* why validate_header refuses it */
  uint32_t algo;                   /* ZKE_SIG_ALGO_* ; meaningful when code is 0 or ZKE_D_NEUTRAL */
  uint32_t sel_off, sel_len;       /* selector bytes in sel_blob; sel_len 0 when there is none */
  uint32_t val_start, val_end;     /* the header's value in raw_email */
  uint32_t reserved;
} zke_sig_info;

/* Where a scan goes: caller-sized buffers, capacities in ENTRIES of the array's type, the sizes needed written back (the
 * zke_capture_out convention).  scan_status (4 n words) and sig_off (n + 1) have sizes known up front: a call whose buffers are
 * smaller fails at once with ZKE_E_NOMEM and the *_need fields set.  sigs and sel_blob depend on the e-mails (n * max_sigs
 * records always suffice): when one of them is too small the call (zke_batch_wait for the asynchronous form) returns ZKE_E_NOMEM,
 * scan_status and sig_off are delivered all the same — and the records, when only the blob is short — and sigs_need /
 * sel_blob_need say exactly what a second call needs.
 *   scan_status  {status, detail, n_signatures, n_candidates} per e-mail.  status ZKE_OK, or ZKE_PARSE_FAIL / ZKE_UNSUPPORTED with
 *                the detail zke_verify_emails gives the same bytes when parse_mail fails (header block, MIME subparts, more than
 *                ZKE_MAX_HEADERS fields, KELVIN SIGN in from_domain): such an e-mail lists no signature.  n_signatures counts
 *                every DKIM-Signature header of the e-mail, n_candidates those with code 0 — also beyond max_sigs: a list that
 *                was cut shows as n_signatures > sig_off[i + 1] - sig_off[i].
 *   sig_off      CSR over the records: e-mail i's are sigs[sig_off[i] .. sig_off[i + 1]), file order, the first max_sigs
 *   sigs         one record per DKIM-Signature header (case-insensitive name), also those the verify path skips.  The engine's
 *                strictness flags apply as in verification; c=, a= and l= are not part of the filter (generator.rs:25-30)
 *   sel_blob     the FWS-stripped s= values of the records with code 0 or ZKE_D_NEUTRAL (ASCII, at most ZKE_MAX_TAGBUF bytes each),
 *                in no particular order: a string is (sel_off, sel_len) */
typedef struct zke_sig_scan {
  uint32_t*     scan_status; size_t scan_status_cap;
  uint32_t*     sig_off;     size_t sig_off_cap;
  zke_sig_info* sigs;        size_t sigs_cap;
  uint8_t*      sel_blob;    size_t sel_blob_cap;
  size_t scan_status_need, sig_off_need, sigs_need, sel_blob_need;      /* written by the call */
  size_t n_sigs;                                                        /* records delivered = sig_off[n] */
} zke_sig_scan;

/* zke_email_ref.key, key_len and key_type are ignored (key may be NULL).  max_sigs: 1 .. ZKE_SCAN_MAX_SIGS, and n * max_sigs below
 * 2^21 (32-bit selector offsets).  `out` and its buffers must stay valid until the batch has been waited for.  One input image
 * without a key section, one launch (sigscan_kernel), one copy back. */
int zke_scan_signatures(zke_engine* e, const zke_email_ref* emails, uint32_t n, uint32_t max_sigs, zke_sig_scan* out);
int zke_scan_signatures_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, uint32_t max_sigs, zke_sig_scan* out, uint64_t* ticket);

/* One candidate key of zke_select_keys.  key_len == 0: "the fetch failed" (generator.rs:33 `continue`); its record is what
 * verify_email gives an empty key (ZKE_KEY_DECODE_FAIL) and it never passes. */
typedef struct zke_key_ref { const uint8_t* key; size_t key_len; uint32_t key_type; uint32_t reserved; } zke_key_ref;
/* Candidate k of e-mail i is keys[cand_off[i] + k]: the key fetched for the k-th record with code 0 the scan listed
 * (emails[i].key* are ignored).  cand_off[n + 1] must be non-decreasing (ZKE_E_ARG otherwise, before anything is staged).
 *   chosen[i]  the smallest k for which verify_email(emails[i] with that key) is ZKE_OK — the reference's rule: verify_email_with_key
 *              with candidate k's key tries EVERY same-domain signature, so selection is "first key under which the e-mail
 *              verifies" —, with ZKE_SEL_AFTER_UNSUPPORTED when an earlier candidate's record is ZKE_UNSUPPORTED; ZKE_SEL_NONE when
 *              none passes.  Test for ZKE_SEL_NONE first; otherwise the index is the low 31 bits.
 *   out[i]     that verification's whole record (public_key_hash is the chosen key's); when none passes, the record of the
 *              e-mail's last candidate; with no candidate at all a zeroed record with ZKE_DKIM_NOT_PASS / ZKE_D_NEUTRAL.
 * All cand_off[n] (e-mail, key) pairs run as ONE batch of the verify pipeline; the fold "first OK per e-mail" happens on the
 * host when the records arrive (zke_batch_wait).  `out`, `chosen` must stay valid until then; cand_off has been copied. */
int zke_select_keys(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off,
                    const zke_key_ref* keys, zke_result* out, uint32_t* chosen);
int zke_select_keys_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off,
                          const zke_key_ref* keys, zke_result* out, uint32_t* chosen, uint64_t* ticket);

/* ---- DKIM key records: what a resolver returns ("v=DKIM1; k=rsa; p=MIGfMA0G...") -> the (key, key_type) pair that
 * Email.public_key and zke_select_keys take.  The reference does this at helpers/src/dkim.rs:67-111: split at ';', k= and p=,
 * base64, SubjectPublicKeyInfo or PKCS#1 in, PKCS#1 out (public_key_hash is SHA-256 of exactly those bytes, circuits.rs:17).
 * One record per wavefront (keyrec_kernel, csrc/keyrec.hip.h).  A canonical SubjectPublicKeyInfo carries its PKCS#1 key as its
 * tail and DER admits one encoding per value, so the re-encoding is "validate, then take the slice".
 *   ZKE_KEYREC_ARCHIVE  dkim.rs:67-111 restated: value.split(';').map(str::trim); a part that starts with "k=" / "p=" (case-
 *                       sensitive) sets the type / the key text, the last such part wins, nothing inside a value is stripped; an
 *                       empty type is "rsa"; base64 0.22 STANDARD (padding required, trailing bits zero, no white space).
 *                       Trimming is ASCII (\t \n \v \f \r space): ZKE_D_KEYREC_NON_ASCII_EDGE where Unicode trimming could differ.
 *   ZKE_KEYREC_DNS      the TXT record of RFC 6376 3.6.1, in the tag-list grammar of the signature parser (the last tag of a name
 *                       wins; what follows the last well-formed tag-spec is not read): FWS around names and values and inside p=
 *                       and k= is removed; v=, when present, is the first tag and "DKIM1"; k= absent or empty is "rsa"; p= is
 *                       required, empty means revoked; h= s= t= n= are ignored.  From the key text on as above.  This is this
 *                       engine's reading: the reference's DNS path is cfdkim's retrieve_public_key, which is not vendored
 *                       (parity unpinned).  A TXT answer of several character-strings is joined by the caller first.
 * For k=rsa: from_public_key_der, then from_pkcs1_der, then RsaPublicKey::new's range (<= 4096 bits, 2 <= e <= 2^33-1); for
 * k=ed25519 exactly 32 bytes (whether they are a curve point is decided at verification, as in the reference). */
#define ZKE_KEYREC_ARCHIVE 0u
#define ZKE_KEYREC_DNS     1u
#define ZKE_KEYREC_MAX_BYTES 4096u      /* longest record read (an RSA-4096 SubjectPublicKeyInfo is 736 characters) */
typedef struct zke_keyrec_ref { const uint8_t* txt; size_t len; } zke_keyrec_ref;    /* len == 0: the fetch failed (generator.rs:33) */
typedef struct zke_key_info {      /* 16 bytes */
  uint32_t code;                   /* 0: a key | ZKE_D_KEYREC_* */
  uint32_t key_type;               /* ZKE_KEY_RSA / ZKE_KEY_ED25519 as far as the record got (ZKE_KEY_OTHER with ZKE_D_KEYREC_TYPE) */
  uint32_t key_off, key_len;       /* the key in zke_keyrec_out.keys: PKCS#1 DER or 32 raw bytes; key_len 0 unless code is 0 */
} zke_key_info;
/* Where the keys go: caller-sized buffers, capacities in ENTRIES, the sizes needed written back (the zke_sig_scan convention).
 * infos (m entries) has a size known up front: too small fails at once with ZKE_E_NOMEM and infos_need set.  keys depends on the
 * records (3/4 of the records' bytes always suffice): when it is too small the call (zke_batch_wait for the asynchronous form)
 * returns ZKE_E_NOMEM, infos is delivered all the same (key_off as it will be) and keys_need says what a second call needs. */
typedef struct zke_keyrec_out {
  zke_key_info* infos; size_t infos_cap;
  uint8_t*      keys;  size_t keys_cap;
  size_t infos_need, keys_need;            /* written by the call */
} zke_keyrec_out;
/* The building block: one image of m records, one launch, infos and key bytes back in one copy.  `out` and its buffers must stay
 * valid until the batch has been waited for; the records have been read when the call returns.  Same slots, tickets and
 * zke_batch_wait as zke_verify_emails_async. */
int zke_decode_key_records(zke_engine* e, const zke_keyrec_ref* recs, uint32_t m, uint32_t mode, zke_keyrec_out* out);
int zke_decode_key_records_async(zke_engine* e, const zke_keyrec_ref* recs, uint32_t m, uint32_t mode, zke_keyrec_out* out, uint64_t* ticket);
/* zke_select_keys with records in place of keys: candidate k of e-mail i is recs[cand_off[i] + k].  The decode launch runs on the
 * batch's slot in front of the front end and leaves the candidates' keys as a packed CSR in HBM, where the verify launches read
 * them: the decoded keys do not visit the host on their way to verification.  A candidate whose record yields no key gets the
 * record verify_email gives an empty RSA key (ZKE_KEY_DECODE_FAIL) and never passes.  chosen, out and the fold on delivery are
 * zke_select_keys'.  keys_out delivers every candidate's info and bytes (cand_off[n] - cand_off[0] infos), so that the caller
 * builds Email.public_key from the chosen one.  Checked before anything is staged: null pointers, cand_off order, mode, and
 * ZKE_E_NOMEM with infos_need set. */
int zke_select_keys_from_records(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off,
                                 const zke_keyrec_ref* recs, uint32_t mode, zke_result* out, uint32_t* chosen, zke_keyrec_out* keys_out);
int zke_select_keys_from_records_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const uint32_t* cand_off,
                                       const zke_keyrec_ref* recs, uint32_t mode, zke_result* out, uint32_t* chosen,
                                       zke_keyrec_out* keys_out, uint64_t* ticket);

/* ---- extract_email_body (core/src/email.rs:7-23, public through `pub use email::*`): the body a reader sees — the text/html part
 * with its Content-Transfer-Encoding undone — for whole batches, one e-mail per wavefront (body_extract_kernel, csrc/bodyext.hip.h).
 * Per e-mail, parse_mail(raw).unwrap() then extract_email_body(&parsed).  This is this engine's reading: mailparse 0.15.0,
 * data-encoding and quoted_printable are not vendored and the rules below are restated from recollection (parity unpinned,
 * DESIGN.md 4; tests/golden/body_manifest.json lists the e-mails that sit on the unverified behaviours).
 *  1. The parse verdict is the verify path's: the same header split and MIME walk, ZKE_PARSE_FAIL / ZKE_UNSUPPORTED with the same
 *     details.  No parse rule is added or changed.
 *  2. Candidates are the DIRECT subparts the walk finds under the message; nested ones are not.
 *  3. A subpart's mimetype: its first Content-Type header (eq_ignore_ascii_case), unfolded as get_value does, the first ';'-token,
 *     trimmed, ASCII-lower-cased; none: text/plain.  (A first token with a byte >= 0x80 or "=?" is the walk's ZKE_D_U_MIME_CTYPE.)
 *  4. The first subpart whose mimetype is "text/html", else the first subpart, else the message itself.
 *  5. body_bytes of that part P: from the end of its header block to its end; when P is itself a multipart whose first boundary
 *     line is found, up to that line (its preamble).  Where the end is a boundary line — P's own end as a subpart, the end of a
 *     preamble — it is moved back over one LF and then one CR in front of it, never past the start.  ZKE_BODYF_PART_KEEPS_EOL
 *     leaves that end alone; the flag moves nothing but the end of the span and never changes a verdict.
 *  6. P's first Content-Transfer-Encoding header, get_value, ASCII-lower-cased, compared WHOLE (no trimming): "base64",
 *     "quoted-printable", anything else or none: identity.  A value with a byte >= 0x80 or "=?": ZKE_UNSUPPORTED / ZKE_D_U_BODY_CTE.
 *  7. Identity: the bytes as they are.
 *  8. Base64: every u8::is_ascii_whitespace byte (HT LF FF CR SP; not VT) is dropped, the rest is strict RFC 4648, standard
 *     alphabet, padding required, trailing bits zero (as ZKE_KEYREC_ARCHIVE).  A failure is get_body_raw().unwrap()'s panic:
 *     ZKE_BODY_DECODE_FAIL with ZKE_D_BODY_B64_CHAR, else _LENGTH, else _TRAILING_BITS (the first that applies, in this order).
 *  9. Quoted-printable (quoted_printable::decode(.., Robust)), never fails: (a) bytes other than HT CR LF and 0x20..0x7E are dropped;
 *     (b) lines as str::lines() (at LF, one CR in front of it removed, a final empty piece is no line); (c) each line's end is
 *     trimmed (SP HT CR); (d) '=' as a line's last character is a soft break: no line break follows the line; (e) '=' and ONE
 *     character at the end of a line are both literal; (f) '=' and two hex digits of either case are that byte; (g) '=' and two
 *     characters that are not both hex are all three literal, and an '=' among the two starts nothing; (h) a line that ended
 *     normally owes one CRLF, paid when another line follows and only then.
 *     "a=\r\nb" -> "ab"; "a \t\r\nb\r\n" -> "a\r\nb"; "=4" -> "=4"; "=zz=41" -> "=zzA"; "==41" -> "==41"; "\r\n\r\n" -> "\r\n".
 *     (A lone LF becomes CRLF: a decoded body can be LONGER than its source, up to twice.)
 * Only raw / raw_len of each zke_email_ref are read.  Slots, tickets and zke_batch_wait are zke_decode_key_records': infos (n
 * entries) too small fails at once with ZKE_E_NOMEM and infos_need set; bytes too small returns ZKE_E_NOMEM (zke_batch_wait for the
 * asynchronous form) with the infos delivered all the same, body_off as it will be and bytes_need exact.  Checked before anything
 * is staged: null pointers, unknown flag bits, an e-mail of 2^31 bytes or more (ZKE_E_ARG). */
#define ZKE_BODYF_PART_KEEPS_EOL 1u
#define ZKE_CTE_IDENTITY 0u
#define ZKE_CTE_BASE64   1u
#define ZKE_CTE_QP       2u
typedef struct zke_body_info {     /* 40 bytes */
  uint32_t status, detail;         /* ZKE_OK | ZKE_PARSE_FAIL | ZKE_BODY_DECODE_FAIL | ZKE_UNSUPPORTED */
  uint32_t part;                   /* 0: the message itself; k >= 1: its k-th direct subpart; bit 31: chosen as text/html */
  uint32_t encoding;               /* ZKE_CTE_* */
  uint32_t src_off, src_len;       /* body_bytes of the chosen part inside the raw e-mail (before decoding) */
  uint32_t body_len, reserved;     /* decoded length; 0 unless status is ZKE_OK */
  uint64_t body_off;               /* into zke_body_out.bytes */
} zke_body_info;                   /* part, encoding, src_off, src_len: as far as the e-mail got (0 with a parse verdict) */
typedef struct zke_body_out {
  zke_body_info* infos; size_t infos_cap;
  uint8_t*       bytes; size_t bytes_cap;
  size_t infos_need, bytes_need;           /* written by the call */
} zke_body_out;
int zke_extract_bodies(zke_engine* e, const zke_email_ref* emails, uint32_t n, uint32_t flags, zke_body_out* out);
int zke_extract_bodies_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, uint32_t flags, zke_body_out* out, uint64_t* ticket);

/* ---- the verifier outputs encoded on the device: per e-mail VerificationOutput::from_parts(email, matches).abi_encode()
 * (core/src/io.rs:28-44; the layout: zke_abi_encode below) — the bytes a zkVM front end commits as public values — and their SHA-256,
 * the value a proof binds to.  One e-mail per wavefront (encode_outputs_kernel, csrc/encode.hip.h), then the engine's ordinary hash
 * launch over the encodings; both follow the verify launches on the batch's stream.
 *   zke_verify_emails_encoded   runs the pipeline of zke_verify_emails (in == NULL, or both of its lists NULL), of
 *                               zke_verify_emails_with_regex (in->lists) or of zke_verify_emails_mixed (in->mixed); out[i] is byte for
 *                               byte the record that entry gives.  An e-mail whose record is ZKE_OK is encoded: kind 0
 *                               (SolEmailOutput) where it is verify_email only — no list form, or config_of[i] == ZKE_CONFIG_NONE —,
 *                               else kind 1 (SolEmailWithRegexOutput), whose matches are ALL its parts' capture strings in part order
 *                               (circuits.rs:58-62): with `lists` the strings cap_off[i * P] .. cap_off[(i + 1) * P], with `mixed`
 *                               cap_off[job_off[i]] .. cap_off[job_off[i + 1]]; possibly none.  Any other status: not encoded —
 *                               len 0, a zero digest, its place in `bytes` left as it was.  external_input_null stays in
 *                               zke_email_ref: such an e-mail reports ZKE_EXTERNAL_INPUT_NULL as always and is not encoded.
 *   external inputs             flattened as the reference does, [name1, value1, name2, value2, ...] (circuits.rs:18-27): e-mail i's
 *                               are the strings ext_off[i] .. ext_off[i + 1] of the CSR table ext_str_off / ext_blob.
 * Strings are bytes with lengths and are NOT validated as UTF-8: the reference's Strings are valid by type, a caller that hands
 * over other bytes gets them encoded as they are.
 * Buffers.  The size of an encoding follows from the kind and the string lengths alone, so off, infos_need and bytes_need are exact
 * and are set BEFORE anything is staged: a call whose infos or bytes is too small fails at once with ZKE_E_NOMEM and both *_need
 * set (the zke_body_out protocol, without its second chance: nothing here depends on the e-mails).  E-mail i's place is
 * bytes[off, off + planned length) whatever its verdict; places follow each other in e-mail order without a gap.
 * ZKE_E_ARG, before anything is staged: both lists and mixed set; offsets that decrease (ext_off, ext_str_off, the capture tables);
 * a null table with a non-zero tail (ext_off names strings and ext_str_off is NULL, or they have bytes and ext_blob is NULL);
 * an encoding of 2^32 bytes or more; and whatever the entry chosen by `in` refuses.
 * Slots, tickets and zke_batch_wait are zke_verify_emails_async's; everything `in` points to has been read when the call returns,
 * `out`, `enc` and its buffers must stay valid until the batch has been waited for. */
typedef struct zke_encoded_info {   /* 48 bytes */
  uint64_t off;        /* the e-mail's place in zke_encoded_out.bytes (planned from the inputs' lengths: known before the batch runs) */
  uint32_t len;        /* bytes of the encoding; 0: not encoded (status != ZKE_OK) */
  uint32_t kind;       /* 0 SolEmailOutput, 1 SolEmailWithRegexOutput */
  uint8_t  digest[32]; /* SHA-256 of bytes[off, off+len); zero when len == 0 */
} zke_encoded_info;
typedef struct zke_encoded_out { zke_encoded_info* infos; size_t infos_cap; uint8_t* bytes; size_t bytes_cap;
                                 size_t infos_need, bytes_need; } zke_encoded_out;
typedef struct zke_encode_in {
  const zke_regex_lists* lists;    /* at most one of lists / mixed; both NULL: verify_email for every e-mail (kind 0) */
  const zke_regex_mixed* mixed;    /* kind 0 where config_of[i] == ZKE_CONFIG_NONE, else 1 */
  const uint32_t* ext_off;         /* [n+1] or NULL: no external inputs anywhere; e-mail i's strings ext_off[i] .. ext_off[i+1] */
  const uint32_t* ext_str_off;     /* [n_strings+1] */
  const uint8_t*  ext_blob;
} zke_encode_in;
int zke_verify_emails_encoded(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_encode_in* in, zke_result* out,
                              zke_encoded_out* enc);
int zke_verify_emails_encoded_async(zke_engine* e, const zke_email_ref* emails, uint32_t n, const zke_encode_in* in, zke_result* out,
                                    zke_encoded_out* enc, uint64_t* ticket);

/* ---- extract, repair and encode in one call: from raw e-mails, keys and a part list to the public values.  The pipeline of
 * zke_extract_captures (same records, spans, flags, the one fold), then on the device and on the batch's stream: the captured bytes
 * repaired as String::from_utf8_lossy repairs them (zke_utf8_lossy_batch above has the rule) — the tables are the reference's
 * CompiledRegex.captures, not raw bytes —, the encode plan, the encodings (kind 1, SolEmailWithRegexOutput, for every e-mail: its
 * matches are all its strings in part order) and their SHA-256.  No table crosses the link twice and no second pipeline runs.
 *   caps    as zke_extract_captures fills it, but cap_str_off / cap_blob hold the REPAIRED strings; flags keep ZKE_CAPF_NOT_UTF8
 *           for the strings that were repaired; spans describe the haystack, not the string, and are unchanged.  May be NULL: the
 *           caller wants the public values only (the tables then never leave the device).  Nobody names a capacity for the
 *           strings then, so the slot's device blob is sized by what they cannot exceed, 3 * min(n * G * ZKE_CAP_MAX_SPAN,
 *           G * (the raw e-mails' bytes + 64 n)) — a buffer that only grows and stays with the slot; a caller that minds the
 *           memory passes a caps whose cap_blob_cap is its own guess and takes the ZKE_E_NOMEM path when it was short.
 *   ext_*   the external inputs, as in zke_encode_in (ext_off NULL: none anywhere).
 *   enc     infos (n entries: too small fails at once with ZKE_E_NOMEM and infos_need set) and bytes.  The plan is made on the device,
 *           which knows the verdicts: an e-mail whose record is not ZKE_OK has len 0, a zero digest and NO place — off is the running
 *           offset and its neighbours' places close up (zke_verify_emails_encoded, planned on the host, leaves such a place unused).
 *           The sizes depend on the e-mails, so bytes follows the cap_blob protocol: when bytes is too small for the encodings, or
 *           cap_blob for the strings, the call (zke_batch_wait for the asynchronous form) returns ZKE_E_NOMEM; records, infos, spans,
 *           flags and both offset tables are delivered all the same, bytes_need and cap_blob_need are exact — one second call
 *           suffices —, an e-mail that did not fit (its place would end beyond bytes_cap, or its strings beyond cap_blob_cap) is
 *           not written and reports len 0 and a zero digest at its planned off — the caller's bytes stay as they were there —, and
 *           nothing is written beyond a capacity.
 * ZKE_E_ARG before anything is staged: what zke_extract_captures refuses; what zke_encode_in's external-input table is refused for;
 * n * G * 3 * ZKE_CAP_MAX_SPAN >= 2^32 (offsets are 32-bit and a repaired string is at most three times its span: n * G >= 349 526);
 * an e-mail whose external inputs, encoded, plus the largest matches its part list can yield (G strings of 3 * ZKE_CAP_MAX_SPAN
 * bytes) would reach 2^32 bytes — so no encoding the device plans can reach that size, which the host plan refuses per call.
 * Slots, tickets and zke_batch_wait are zke_extract_captures_async's; zke_timings has no new field (the launches count as the regex
 * stage's).  Not built: a form over mixed configs (zke_extract_captures_mixed keeps raw bytes and the two-call path), a form over
 * device-resident e-mails; zke_extract_captures* deliver raw bytes as before. */
int zke_extract_captures_encoded(zke_engine* e, const zke_email_ref* emails, uint32_t n,
                                 const zke_capture_part* header_parts, uint32_t n_header_parts,
                                 const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out, zke_capture_out* caps,
                                 const uint32_t* ext_off, const uint32_t* ext_str_off, const uint8_t* ext_blob, zke_encoded_out* enc);
int zke_extract_captures_encoded_async(zke_engine* e, const zke_email_ref* emails, uint32_t n,
                                       const zke_capture_part* header_parts, uint32_t n_header_parts,
                                       const zke_capture_part* body_parts, uint32_t n_body_parts, zke_result* out, zke_capture_out* caps,
                                       const uint32_t* ext_off, const uint32_t* ext_str_off, const uint8_t* ext_blob, zke_encoded_out* enc,
                                       uint64_t* ticket);

/* Device-resident batch: every pointer in `in` and `out_dev` is device memory (the part-id lists stay host arrays);
 * `raw_total`, `domain_total`, `key_total` are the blob sizes (the CSR tails), which the
 * host needs for workspace sizing without a device read.  Takes the engine's next submission slot (round-robin over the
 * hardware queues the slot streams share, then over a queue's slots: zke_engine_slot_queue; plain round-robin while that map is unknown),
 * enqueues on `stream` (a hipStream_t; NULL = that slot's own stream) and returns without synchronising: with S slots
 * reserved, S consecutive calls run concurrently.  A slot is reused only behind its previous batch (stream order, or an
 * event wait when the caller's stream changed).  zke_engine_sync waits for every slot. */
int zke_verify_batch_device(zke_engine* e, const zke_batch* in, uint64_t raw_total,
                            uint64_t domain_total, uint64_t key_total,
                            zke_result* out_dev, void* stream);
int zke_engine_sync(zke_engine* e);
/* Device-side join, no host wait: whatever is enqueued on `stream` (a hipStream_t; here NULL is the device's null stream)
 * after this call runs behind every batch submitted so far, on whichever slot or stream it went.  For a consumer of the
 * result records that lives on a stream of its own (a copy, a collective): it can be enqueued while the batches still run. */
int zke_engine_join(zke_engine* e, void* stream);
/* Timings of the last batch that ran in `slot` / in the slot used most recently.  A slot that has not run a timed batch
 * reports all zeros. */
int zke_get_timings(zke_engine* e, zke_timings* t);
int zke_get_slot_timings(zke_engine* e, uint32_t slot, zke_timings* t);
/* Which two-wave SHA-256 routine the engine's hash launches take as it stands now: 1 the ring (two K+W buffers), 0 the pair
 * (one).  Chosen like the eight-lane RSA role — min(slots that exist, GPU_MAX_HW_QUEUES as read at creation) <= 4 takes the
 * ring — or forced by ZKE_SHA_RING = 0 / 1 in the environment at zke_engine_create.  Negative: an error code. */
int zke_engine_sha_ring(zke_engine* e);
/* The lane mapping of the ring's rounds wave as the engine stands now: 1 two lanes per message (the twin: groups of 32 messages, for
 * bodies and header preimages in the hash / modexp launch and for zke_sha256_batch), 0 one lane per message.  1 only where
 * zke_engine_sha_ring answers 1; ZKE_SHA_TWIN = 0 / 1 in the environment at zke_engine_create turns it off / asks for it wherever the
 * ring is taken.  Negative: an error code. */
int zke_engine_sha_twin(zke_engine* e);
/* Whether the round-0 front end of a batch of n e-mails runs two waves per e-mail as the engine stands now: 1 a helper wave
 * canonicalises the body beside the header-hash preimage, 0 one wave does both.  Chosen like the ring — min(slots that exist,
 * GPU_MAX_HW_QUEUES as read at creation) <= 4 — for batches of at most 1 024 e-mails, or forced by ZKE_FRONT_HELPER = 0 / 1 in the
 * environment at zke_engine_create.  Negative: an error code. */
int zke_engine_front_helper(zke_engine* e, uint32_t n);
/* Which slots share a hardware queue, as zke_engine_reserve read it from the device (HIP places the slot streams on GPU_MAX_HW_QUEUES
 * queues, and a queue runs its kernels one after the other).  zke_engine_queue_count: the number of groups, 0 while the map is unknown
 * (before the first zke_engine_reserve, or when every slot has a queue to itself); negative: an error code.  zke_engine_slot_queue: the
 * group of `slot`, numbered in order of the groups' lowest slot index, or -1 if unknown.  Submission ticket t (counted from the engine's
 * creation, every entry point) goes to group t % count and takes that group's slots in turn, in ascending slot index: every queue gets
 * the same share of the batches however many slots sit on it.  With the map unknown ticket t goes to slot t % slots.
 * zke_engine_last_slot: the slot the most recent submission took (the one zke_get_timings reads); negative: an error code. */
int zke_engine_queue_count(zke_engine* e);
int zke_engine_slot_queue(zke_engine* e, uint32_t slot);
int zke_engine_last_slot(zke_engine* e);
/* Enable per-launch HIP-event timing (adds event records between the launches). */
int zke_set_timing(zke_engine* e, int enabled);

/* Single-email wrappers over a batch of one (config 1 / API-shape parity): the two functions of the reference,
 *     verify_email(&Email)                      core/src/circuits.rs:9
 *     verify_email_with_regex(&EmailWithRegex)  core/src/circuits.rs:31
 * with the struct fields spelled out as pointers and sizes.  `external_input_null` != 0: some ExternalInput.value is
 * None (circuits.rs:24 panics after the DKIM assert and before any regex work; the status order is the reference's). */
int zke_verify_email(zke_engine* e, const uint8_t* raw, size_t raw_len,
                     const char* from_domain, size_t domain_len,
                     const uint8_t* key, size_t key_len, uint32_t key_type,
                     uint32_t external_input_null, zke_result* out);

/* One CompiledRegex of RegexInfo.header_parts / body_parts (core/src/structs.rs:16-35). */
typedef struct zke_regex_part {
  const uint8_t* fwd; size_t fwd_len;        /* verify_re.fwd: regex-automata dense DFA, little-endian, padding stripped */
  const uint8_t* bwd; size_t bwd_len;        /* verify_re.bwd */
  uint32_t n_captures;                       /* captures: Some(v) -> v.len(); None -> 0 (core/src/regex.rs:41 skips the check) */
  const uint8_t* const* captures;            /* [n_captures] UTF-8 bytes, no terminator needed */
  const size_t* capture_lens;                /* [n_captures] */
} zke_regex_part;

/* Registers the DFA pairs it has not seen before (zke_dfa_register returns the old id for an equal pair), so calling
 * this per e-mail with the same regex_config parses every table once, not once per e-mail as core/src/regex.rs:32-33.
 * Pairs registered this way are the ones the registry evicts (least recently used first) when it is full. */
int zke_verify_email_with_regex(zke_engine* e, const uint8_t* raw, size_t raw_len,
                                const char* from_domain, size_t domain_len,
                                const uint8_t* key, size_t key_len, uint32_t key_type,
                                uint32_t external_input_null,
                                const zke_regex_part* header_parts, uint32_t n_header_parts,
                                const zke_regex_part* body_parts, uint32_t n_body_parts,
                                zke_result* out);

/* ---- serialised inputs -------------------------------------------------------------------------
 * The byte streams the zkVM hosts already produce for Email / EmailWithRegex (the derives at core/src/structs.rs:1-6): borsh
 * under the reference's `risc0` feature (u32 lengths), bincode 1.x default options over serde under `sp1` (u64 lengths).  Read
 * in place — every pointer of a zke_wire_email points into the caller's buffer, which must outlive the document. */
#define ZKE_WIRE_BORSH   0u
#define ZKE_WIRE_BINCODE 1u
typedef struct zke_wire_doc zke_wire_doc;
typedef struct zke_wire_email {                 /* Email (structs.rs:49-54) + RegexInfo (structs.rs:32-35) as the entry points take them */
  const uint8_t* raw; size_t raw_len;           /* Email.raw_email */
  const char* from_domain; size_t domain_len;   /* Email.from_domain (UTF-8, validated) */
  const uint8_t* key; size_t key_len;           /* Email.public_key.key */
  uint32_t key_type;                            /* ZKE_KEY_* of Email.public_key.key_type */
  uint32_t n_external_inputs;                   /* Email.external_inputs.len(); zke_wire_external_input reads one */
  uint32_t external_input_null;                 /* 1: some ExternalInput.value is None (circuits.rs:24) */
  uint32_t has_header_parts, has_body_parts;    /* Option tags of RegexInfo.header_parts / body_parts */
  uint32_t n_header_parts, n_body_parts;
  const zke_regex_part* header_parts;           /* [n_header_parts]; captures: None -> n_captures 0 */
  const zke_regex_part* body_parts;
} zke_wire_email;
/* Decode ONE record at bytes[0, len): Email (with_regex == 0) or EmailWithRegex.  *consumed = its size (records may follow
 * each other in a stream).  ZKE_E_ARG with a message (zke_last_error(NULL)) for a truncated or malformed stream. */
int zke_wire_decode(uint32_t format, const uint8_t* bytes, size_t len, uint32_t with_regex, zke_wire_doc** out, size_t* consumed);
void zke_wire_free(zke_wire_doc* d);
int zke_wire_view(const zke_wire_doc* d, zke_wire_email* out);
int zke_wire_external_input(const zke_wire_doc* d, uint32_t i, const uint8_t** name, size_t* name_len,
                            const uint8_t** value, size_t* value_len, uint32_t* is_null);
/* verify_email / verify_email_with_regex of one serialised record: decode + zke_verify_email[_with_regex].  The record must
 * fill bytes[0, len) exactly. */
int zke_verify_wire(zke_engine* e, uint32_t format, const uint8_t* bytes, size_t len, uint32_t with_regex, zke_result* out);

/* ---- one batch over N GPUs ----------------------------------------------------------------------------
 * Every e-mail is verified in isolation, so ranks take contiguous ranges of a batch balanced by cumulative raw BYTES (not by
 * count: a ragged batch then loads the ranks evenly) and the data path has no collective; the only exchange is the gather of
 * the per-e-mail witnesses.  zke_shard_bounds writes bounds[0 .. world]: rank r owns e-mails [bounds[r], bounds[r + 1]) of the
 * n whose CSR offsets are raw_off[0 .. n]; cut points sit where the cumulative byte count crosses r / world of the total.
 * Rank r then runs zke_verify_batch_device on its range — the offsets are absolute, so a range is `raw_off + bounds[r]` with
 * the same blobs — and contributes (bounds[r + 1] - bounds[r]) records.  Pure host code.  (Python:
 * zkemail_rs_amd.distributed.shard_bounds / ShardedVerifier, the latter with the RCCL all-gather of the witnesses.) */
int zke_shard_bounds(const uint64_t* raw_off, uint32_t n, uint32_t world, uint32_t* bounds);

/* Building blocks, exported for parity tests and micro-benchmarks.  Host pointers. */
/* n messages msg_blob[off[i]..off[i+1]) -> digests[32*i..]           (core/src/crypto.rs:3-7) */
int zke_sha256_batch(zke_engine* e, const uint8_t* msg_blob, const uint64_t* off,
                     uint32_t n, uint8_t* digests);
/* n RSA public-key operations: em[i] = sig[i]^e[i] mod n[i].  sig/mod big-endian,
 * `bytes` each (<= 512, multiple of 4); em big-endian `bytes` each.  ok[i] = 0 when
 * sig >= n or n even.  */
int zke_rsa_modexp_batch(zke_engine* e, const uint8_t* sig, const uint8_t* mod,
                         const uint64_t* exp, uint32_t bytes, uint32_t n,
                         uint8_t* em, uint8_t* ok);
/* n independent Ed25519 verifications under the rule cfdkim applies to k=ed25519 keys (ed25519-dalek 2.1.1
 * verify_strict, Cargo.lock:778).  keys n x 32 bytes, msgs n x msg_len bytes (msg_len <= 32: DKIM signs the
 * 32-byte header hash), sigs n x 64 bytes.  out[i]: 0 = key does not decode to a curve point
 * (VerifyingKey::from_bytes fails), 1 = signature rejected, 2 = valid. */
int zke_ed25519_verify_batch(zke_engine* e, const uint8_t* keys, const uint8_t* msgs, uint32_t msg_len,
                             const uint8_t* sigs, uint32_t n, uint32_t* out);
/* Device-resident SHA-256 micro-benchmark entry: messages already in HBM. */
int zke_sha256_batch_device(zke_engine* e, const uint8_t* msg_blob_dev, const uint64_t* off_dev,
                            uint32_t n, uint8_t* digests_dev, void* stream);

/* The encode and digest launches of zke_verify_emails_encoded alone, over records and tables of the caller's (host pointers): for
 * parity tests, and for a caller that already holds a batch's records.  records[n]: status, from_domain_hash and public_key_hash are
 * read; kinds[n]: 0 / 1 as zke_encoded_info.kind.  Two CSR string tables of the same shape: e-mail i's external inputs are the
 * strings ext_off[i] .. ext_off[i + 1] of ext_str_off / ext_blob, its matches (kind 1 only) the strings match_off[i] ..
 * match_off[i + 1] of match_str_off / match_blob; ext_off / match_off NULL: none anywhere.  `enc`, the checks (ZKE_E_ARG, also for a
 * kind above 1) and the exact sizes (ZKE_E_NOMEM at once) are zke_verify_emails_encoded's.  Synchronous; runs in one slot, whose
 * output buffer is the one that entry uses. */
int zke_encode_outputs(zke_engine* e, const zke_result* records, uint32_t n, const uint32_t* kinds,
                       const uint32_t* ext_off, const uint32_t* ext_str_off, const uint8_t* ext_blob,
                       const uint32_t* match_off, const uint32_t* match_str_off, const uint8_t* match_blob, zke_encoded_out* enc);

/* Solidity ABI encoding of a verifier output — what VerificationOutput::from_parts(email, matches).abi_encode()
 * returns (core/src/io.rs:28-44): abi.encode of
 *     struct SolEmailOutput          { bytes32 from_domain_hash; bytes32 public_key_hash; string[] external_inputs; }
 *     struct SolEmailWithRegexOutput { SolEmailOutput email; string[] matches; }               (core/src/io.rs:5-16)
 * with_matches == 0: EmailOnly; != 0: WithRegex (matches may then be empty).  Strings are UTF-8 bytes with lengths.
 * Pure host code, no engine and no GPU.  Writes *out_len = the encoding's size; returns ZKE_E_NOMEM (nothing written)
 * when out_cap is smaller — call with out == NULL, out_cap == 0 to size the buffer. */
int zke_abi_encode(const uint8_t* from_domain_hash /*[32]*/, const uint8_t* public_key_hash /*[32]*/,
                   const uint8_t* const* external_inputs, const size_t* external_input_lens, uint32_t n_external_inputs,
                   uint32_t with_matches, const uint8_t* const* matches, const size_t* match_lens, uint32_t n_matches,
                   uint8_t* out, size_t out_cap, size_t* out_len);

/* Library / build identification.  zke_abi_version() = 3 for this header (struct layouts and entry points of ABI 0.3). */
const char* zke_version(void);
uint32_t zke_abi_version(void);
/* The reference panic site a status stands for, as text ("assert!(verified)  core/src/circuits.rs:13"); "" for ZKE_OK,
 * "unknown status" beyond the enum.  A static string. */
const char* zke_status_name(uint32_t status);
/* 1 if a HIP device is usable from this process, else 0 (never falls back to a CPU path). */
int zke_device_available(void);

#ifdef __cplusplus
}
#endif
#endif /* ZKEMAIL_AMD_H */
