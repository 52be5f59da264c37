//! `zkemail-core-amd` — zkemail-core's verification API over the MI355X-native batched engine.
//!
//! ```ignore
//! // before:  use zkemail_core::{verify_email, verify_email_with_regex};
//! use zkemail_core_amd::{verify_email, verify_email_with_regex};
//! ```
//!
//! Same input and output structs (they are re-exported from `zkemail-core`, `core/src/structs.rs:8-75`), same
//! function signatures (`core/src/circuits.rs:9,31`) and the same failure behaviour: where the reference panics
//! (`assert!` `circuits.rs:13,45,54`; `expect` `:24`; `unwrap` `circuits.rs:35`, `email.rs:26,29,33`,
//! `regex.rs:32,33`) these functions panic too, with a message that names the site.  What differs is where the
//! work happens: header split, canonicalisation, SHA-256, RSA / Ed25519 and the DFA walk run on the GPU behind
//! `libzkemail_amd.so`.  A GPU pays off on batches, so the crate adds [`Engine::verify_emails`] /
//! [`Engine::verify_emails_with_regex`], which take slices and return one `Result` per e-mail instead of aborting
//! the batch on the first bad one.
//!
//! No Rust toolchain exists in the image this repository is built in: the crate is source that mirrors
//! `include/zkemail_core.hpp` (its compiled and GPU-tested C++ twin) call for call, and
//! `tests/test_rust_bindings.py` keeps the FFI layer under it identical to the C header.
#![deny(unsafe_op_in_unsafe_fn)]

use std::ffi::CStr;
use std::fmt;
use std::ptr;
use std::sync::OnceLock;

use zkemail_amd_sys as sys;

pub use zkemail_core::{
    hash_bytes, remove_quoted_printable_soft_breaks, CompiledRegex, Email, EmailVerifierOutput, EmailWithRegex,
    EmailWithRegexVerifierOutput, ExternalInput, PublicKey, RegexInfo, VerificationOutput, DFA,
};

/// The reference would have panicked on this e-mail: `status` names the panic site
/// (`ZKE_PARSE_FAIL` = `email.rs:26` … `ZKE_BODY_REGEX_FAIL` = `circuits.rs:54`), `detail` is cfdkim's reason.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct Panic {
    pub status: u32,
    pub detail: u32,
}

impl Panic {
    /// The reference source line whose `assert!` / `unwrap` / `expect` fires for this status.
    pub fn site(&self) -> &'static str {
        match self.status {
            sys::ZKE_PARSE_FAIL => "core/src/email.rs:26 mailparse::parse_mail(..).unwrap()",
            sys::ZKE_KEY_DECODE_FAIL => "core/src/email.rs:29 DkimPublicKey::try_from_bytes(..).unwrap()",
            sys::ZKE_DKIM_ERROR => "core/src/email.rs:33 verify_email_with_key(..).unwrap()",
            sys::ZKE_DKIM_NOT_PASS => "core/src/circuits.rs:13 assert!(verified)",
            sys::ZKE_EXTERNAL_INPUT_NULL => "core/src/circuits.rs:24 expect(\"Value cannot be null\")",
            sys::ZKE_CANON_FAIL => "core/src/circuits.rs:35 canonicalize_signed_email(..).unwrap()",
            sys::ZKE_DFA_DECODE_FAIL => "core/src/regex.rs:32-33 dense::DFA::from_bytes(..).unwrap()",
            sys::ZKE_HEADER_REGEX_FAIL => "core/src/circuits.rs:45 assert!(verified)",
            sys::ZKE_BODY_REGEX_FAIL => "core/src/circuits.rs:54 assert!(verified)",
            sys::ZKE_UNSUPPORTED => "input outside what the engine implements (never a silent mis-verify)",
            sys::ZKE_BODY_DECODE_FAIL => "core/src/email.rs:17-21 part.get_body_raw().unwrap() in extract_email_body",
            _ => "unknown status",
        }
    }
}

impl fmt::Display for Panic {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "zkemail_core would panic at {} (status {}, detail {})", self.site(), self.status, self.detail)
    }
}

impl std::error::Error for Panic {}

/// The call itself failed (no GPU, bad arguments, out of device memory) — not a property of an e-mail.
#[derive(Debug, Clone)]
pub struct EngineError {
    pub code: i32,
    pub message: String,
}

impl fmt::Display for EngineError {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "zkemail_amd engine error {}: {}", self.code, self.message)
    }
}

impl std::error::Error for EngineError {}

/// One DKIM-Signature header as a scan reports it (`zke_sig_info`, the selector as a string: it is ASCII by construction).
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct SigInfo {
    pub header_index: u32,
    pub code: u32,
    pub algo: u32,
    pub selector: String,
    pub value_span: (u32, u32),
}

/// One DKIM key record as a decode reports it (`zke_key_info`, the key as bytes): `code` 0 and the key, or `ZKE_D_KEYREC_*`.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct KeyInfo {
    pub code: u32,
    pub key_type: u32,
    pub key: Vec<u8>,
}

impl KeyInfo {
    /// `Email.public_key` of a record that decoded.
    pub fn public_key(&self) -> PublicKey {
        PublicKey { key: self.key.clone(), key_type: if self.key_type == sys::ZKE_KEY_ED25519 { "ed25519".into() } else { "rsa".into() } }
    }
}

/// A scan's answer for one e-mail; `sigs` holds the first `max_sigs` headers, the counts are the true ones.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct SigScan {
    pub status: u32,
    pub detail: u32,
    pub n_signatures: u32,
    pub n_candidates: u32,
    pub sigs: Vec<SigInfo>,
}

/// One `Email` as the C side sees it: pointers into its own buffers (valid while the `Email` is borrowed).
fn email_ref(e: &Email) -> sys::zke_email_ref {
    sys::zke_email_ref {
        raw: e.raw_email.as_ptr(),
        raw_len: e.raw_email.len(),
        from_domain: e.from_domain.as_ptr() as *const std::os::raw::c_char,
        domain_len: e.from_domain.len(),
        key: e.public_key.key.as_ptr(),
        key_len: e.public_key.key.len(),
        key_type: key_type_code(&e.public_key.key_type) as u32,
        external_input_null: e.external_inputs.iter().any(|x| x.value.is_none()) as u32,
    }
}

fn key_type_code(key_type: &str) -> u8 {
    match key_type {
        "rsa" => sys::ZKE_KEY_RSA as u8,
        "ed25519" => sys::ZKE_KEY_ED25519 as u8,
        _ => sys::ZKE_KEY_OTHER as u8, // DkimPublicKey::try_from_bytes rejects it: ZKE_KEY_DECODE_FAIL
    }
}

/// Struct-of-arrays image of `&[Email]` as `zke_batch` wants it (CSR blobs, `include/zkemail_amd.h`).  `verify_emails` does not
/// need it (the engine gathers the e-mails from where they are); it is for a caller that submits the same batch more than once
/// or uploads it to HBM for `zke_verify_batch_device` (`Engine::verify_packed`).
pub struct Packed {
    raw_blob: Vec<u8>,
    raw_off: Vec<u64>,
    domain_blob: Vec<u8>,
    domain_off: Vec<u64>,
    key_blob: Vec<u8>,
    key_off: Vec<u64>,
    key_type: Vec<u8>,
    ext_null: Vec<u8>,
}

impl Packed {
    pub fn from_emails<'a, I: Iterator<Item = &'a Email>>(emails: I) -> Self {
        let mut p = Packed {
            raw_blob: Vec::new(),
            raw_off: vec![0],
            domain_blob: Vec::new(),
            domain_off: vec![0],
            key_blob: Vec::new(),
            key_off: vec![0],
            key_type: Vec::new(),
            ext_null: Vec::new(),
        };
        for e in emails {
            p.raw_blob.extend_from_slice(&e.raw_email);
            p.raw_off.push(p.raw_blob.len() as u64);
            p.domain_blob.extend_from_slice(e.from_domain.as_bytes());
            p.domain_off.push(p.domain_blob.len() as u64);
            p.key_blob.extend_from_slice(&e.public_key.key);
            p.key_off.push(p.key_blob.len() as u64);
            p.key_type.push(key_type_code(&e.public_key.key_type));
            // circuits.rs:24: a None value panics — after the DKIM assert, before any regex work
            p.ext_null.push(e.external_inputs.iter().any(|x| x.value.is_none()) as u8);
        }
        // the C side never dereferences an empty blob, but it wants non-null pointers
        for blob in [&mut p.raw_blob, &mut p.domain_blob, &mut p.key_blob] {
            if blob.is_empty() {
                blob.push(0);
            }
        }
        p
    }

    pub fn batch(&self, n: usize) -> sys::zke_batch {
        sys::zke_batch {
            n: n as u32,
            raw_blob: self.raw_blob.as_ptr(),
            raw_off: self.raw_off.as_ptr(),
            domain_blob: self.domain_blob.as_ptr(),
            domain_off: self.domain_off.as_ptr(),
            key_blob: self.key_blob.as_ptr(),
            key_off: self.key_off.as_ptr(),
            key_type: self.key_type.as_ptr(),
            ext_null: self.ext_null.as_ptr(),
            with_regex: 0,
            n_header_parts: 0,
            n_body_parts: 0,
            header_part_ids: ptr::null(),
            body_part_ids: ptr::null(),
            cap_off: ptr::null(),
            cap_str_off: ptr::null(),
            cap_blob: ptr::null(),
        }
    }
}

fn zeroed_result() -> sys::zke_result {
    sys::zke_result {
        status: 0,
        detail: 0,
        sig_index: 0,
        flags: 0,
        canon_header_len: 0,
        canon_body_len: 0,
        body_offset: 0,
        n_headers: 0,
        from_domain_hash: [0; 32],
        public_key_hash: [0; 32],
        body_hash: [0; 32],
        header_hash: [0; 32],
        regex_part: 0,
        match_count: 0,
        match_start: 0,
        match_end: 0,
        rsa_bits: 0,
        reserved: [0; 3],
    }
}

/// `EmailVerifierOutput` of a verified e-mail (circuits.rs:15-28): the two witnesses come from the record, the
/// external inputs are echoed `[name, value, ...]`.
fn email_output(email: &Email, r: &sys::zke_result) -> EmailVerifierOutput {
    EmailVerifierOutput {
        from_domain_hash: r.from_domain_hash.to_vec(),
        public_key_hash: r.public_key_hash.to_vec(),
        external_inputs: email
            .external_inputs
            .iter()
            .flat_map(|x| vec![x.name.clone(), x.value.clone().expect("Value cannot be null")])
            .collect(),
    }
}

/// `regex_matches` = header captures then body captures (circuits.rs:58-62); the strings are the *input* capture
/// strings (regex.rs:47), meaningful once the engine reported `ZKE_OK`.
fn regex_matches_of(info: &RegexInfo) -> Vec<String> {
    let mut out = Vec::new();
    for parts in [&info.header_parts, &info.body_parts] {
        if let Some(parts) = parts {
            for p in parts {
                if let Some(c) = &p.captures {
                    out.extend(c.iter().cloned());
                }
            }
        }
    }
    out
}

/// The default configuration (a zero-filled `zke_options` with the device set).
pub fn default_options(device: i32) -> sys::zke_options {
    sys::zke_options {
        device,
        slots: 0,
        max_sig_rounds: 0,
        disable_key_cache: 0,
        host_threads: 0,
        max_dfas: 0,
        rsa_lane_groups: 0,
        dfa_mapping: 0,
        replay_graphs: 0,
        enforce_expiry_x: 0,
        canon_takes_verified_signature: 0,
        canon_ignores_l: 0,
        i_must_be_subdomain: 0,
        b_removes_own_span_only: 0,
        sha_mapping: 0,
        now_unix: 0,
        reserved: [0; 4],
    }
}

/// One engine per GPU: submission slots (a stream, a workspace and a pinned staging image each), registered DFA
/// tables, the per-key Montgomery cache.  Re-entrant, as the reference's functions are (core/src/circuits.rs:9): the
/// C entry points take a slot by an atomic ticket and hold that slot's lock while they enqueue, so one `Engine` may be
/// shared by any number of threads.
pub struct Engine {
    raw: *mut sys::zke_engine,
}

// The handle owns device memory and streams; the C-ABI serialises what must be serialised (include/zkemail_amd.h, "Threading").
unsafe impl Send for Engine {}
unsafe impl Sync for Engine {}

impl Engine {
    /// `device`: HIP device ordinal, -1 = the current device.  Every other option at its default.
    pub fn new(device: i32) -> Result<Self, EngineError> {
        Self::with_options(default_options(device))
    }

    /// An engine with explicit `zke_options` (ABI 0.3: submission slots, host threads, kernel variants and the
    /// strictness flags — the readings of cfdkim that a maintainer with the crates at hand may want to flip).
    pub fn with_options(opt: sys::zke_options) -> Result<Self, EngineError> {
        let mut raw: *mut sys::zke_engine = ptr::null_mut();
        // SAFETY: `opt` and `raw` outlive the call; the callee writes a handle or leaves null.
        let rc = unsafe { sys::zke_engine_create(&opt, &mut raw) };
        if rc != 0 || raw.is_null() {
            return Err(EngineError { code: rc, message: "zke_engine_create failed (no HIP device? the engine has no CPU path)".into() });
        }
        Ok(Engine { raw })
    }

    fn last_error(&self, code: i32) -> EngineError {
        // SAFETY: the engine is alive; zke_last_error returns a NUL-terminated string it owns.
        let message = unsafe { CStr::from_ptr(sys::zke_last_error(self.raw)) }.to_string_lossy().into_owned();
        EngineError { code, message }
    }

    /// Pre-size `slots` submission slots for batches of up to `max_n` e-mails / `max_raw_total` raw bytes
    /// (`zke_engine_reserve`): nothing is allocated in the submit path afterwards.
    pub fn reserve(&self, max_n: u32, max_raw_total: u64, slots: u32, max_regex_parts: u32) -> Result<(), EngineError> {
        // SAFETY: plain values.
        let rc = unsafe { sys::zke_engine_reserve(self.raw, max_n, max_raw_total, slots, max_regex_parts) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(())
    }

    /// The raw records of a batch packed beforehand (`Packed::from_emails`): `zke_verify_batch` over the three CSR blobs.
    pub fn verify_packed(&self, packed: &Packed, n: usize) -> Result<Vec<sys::zke_result>, EngineError> {
        let batch = packed.batch(n);
        let mut out = vec![zeroed_result(); n];
        // SAFETY: every pointer in `batch` refers into `packed`, borrowed for the whole (synchronous) call; `out` holds n records.
        let rc = unsafe { sys::zke_verify_batch(self.raw, &batch, out.as_mut_ptr(), ptr::null_mut()) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(out)
    }

    /// `verify_email` over a slice: one `Result` per e-mail, in order.  Never aborts the batch on a bad e-mail.
    pub fn verify_emails(&self, emails: &[Email]) -> Result<Vec<Result<EmailVerifierOutput, Panic>>, EngineError> {
        if emails.is_empty() {
            return Ok(Vec::new());
        }
        // The e-mails stay where they are: one zke_email_ref per `Email`, pointing into its own Vec<u8> / Strings.  The engine
        // gathers them into its pinned staging image on its packing threads (zke_verify_emails) — no concatenation here.
        let refs: Vec<sys::zke_email_ref> = emails.iter().map(email_ref).collect();
        let mut out = vec![zeroed_result(); emails.len()];
        // SAFETY: every pointer in `refs` refers into `emails`, borrowed for the whole (synchronous) call; `out` holds n records.
        let rc = unsafe { sys::zke_verify_emails(self.raw, refs.as_ptr(), refs.len() as u32, out.as_mut_ptr()) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(emails
            .iter()
            .zip(out.iter())
            .map(|(e, r)| if r.status == sys::ZKE_OK { Ok(email_output(e, r)) } else { Err(Panic { status: r.status, detail: r.detail }) })
            .collect())
    }

    /// `verify_email_with_regex` over a slice.  All inputs must share one part list (one `regex_config` per batch:
    /// the same DFA pairs in the same order); the captures are per e-mail.  Each DFA pair is parsed and staged on
    /// the device once (`zke_dfa_register`), not once per e-mail as `core/src/regex.rs:32-33` does.
    pub fn verify_emails_with_regex(
        &self,
        inputs: &[EmailWithRegex],
    ) -> Result<Vec<Result<EmailWithRegexVerifierOutput, Panic>>, EngineError> {
        if inputs.is_empty() {
            return Ok(Vec::new());
        }
        let empty: Vec<CompiledRegex> = Vec::new();
        let first = &inputs[0].regex_info;
        let ids = |engine: &Engine, parts: &Option<Vec<CompiledRegex>>| -> Result<Vec<u32>, EngineError> {
            let mut v = Vec::new();
            for p in parts.as_ref().unwrap_or(&empty) {
                let mut id = 0u32;
                // SAFETY: the slices outlive the call; the engine copies what it keeps.
                let rc = unsafe {
                    sys::zke_dfa_register(
                        engine.raw,
                        p.verify_re.fwd.as_ptr(),
                        p.verify_re.fwd.len(),
                        p.verify_re.bwd.as_ptr(),
                        p.verify_re.bwd.len(),
                        &mut id,
                    )
                };
                if rc != 0 {
                    return Err(engine.last_error(rc));
                }
                v.push(id); // registering an equal pair again returns the id it already has
            }
            Ok(v)
        };
        let hdr_ids = ids(self, &first.header_parts)?;
        let body_ids = ids(self, &first.body_parts)?;
        let n_parts = hdr_ids.len() + body_ids.len();
        // captures: two-level CSR — strings cap_str_off[cap_off[i*P+p] .. cap_off[i*P+p+1]) of e-mail i, part p
        let mut cap_off: Vec<u32> = vec![0];
        let mut cap_str_off: Vec<u32> = vec![0];
        let mut cap_blob: Vec<u8> = Vec::new();
        for inp in inputs {
            if ids(self, &inp.regex_info.header_parts)? != hdr_ids || ids(self, &inp.regex_info.body_parts)? != body_ids {
                return Err(EngineError { code: sys::ZKE_E_ARG, message: "a batch must share one part list; split it per regex_config".into() });
            }
            for parts in [&inp.regex_info.header_parts, &inp.regex_info.body_parts] {
                for p in parts.as_ref().unwrap_or(&empty) {
                    for c in p.captures.as_ref().map(|v| v.as_slice()).unwrap_or(&[]) {
                        cap_blob.extend_from_slice(c.as_bytes());
                        cap_str_off.push(cap_blob.len() as u32);
                    }
                    cap_off.push((cap_str_off.len() - 1) as u32);
                }
            }
        }
        if cap_blob.is_empty() {
            cap_blob.push(0);
        }
        // the e-mails stay in their own buffers (zke_verify_emails_with_regex gathers them); only the small tables are built here
        let refs: Vec<sys::zke_email_ref> = inputs.iter().map(|i| email_ref(&i.email)).collect();
        let lists = sys::zke_regex_lists {
            n_header_parts: hdr_ids.len() as u32,
            header_part_ids: hdr_ids.as_ptr(),
            n_body_parts: body_ids.len() as u32,
            body_part_ids: body_ids.as_ptr(),
            cap_off: if n_parts > 0 { cap_off.as_ptr() } else { ptr::null() },
            cap_str_off: cap_str_off.as_ptr(),
            cap_blob: cap_blob.as_ptr(),
        };
        let mut out = vec![zeroed_result(); inputs.len()];
        // SAFETY: as in verify_emails; the id lists and the capture tables live until the call returns.
        let rc = unsafe { sys::zke_verify_emails_with_regex(self.raw, refs.as_ptr(), refs.len() as u32, &lists, out.as_mut_ptr()) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(inputs
            .iter()
            .zip(out.iter())
            .map(|(inp, r)| {
                if r.status == sys::ZKE_OK {
                    Ok(EmailWithRegexVerifierOutput { email: email_output(&inp.email, r), regex_matches: regex_matches_of(&inp.regex_info) })
                } else {
                    Err(Panic { status: r.status, detail: r.detail })
                }
            })
            .collect())
    }

    /// `verify_email_with_regex` over a slice as the reference has it: every value with a `RegexInfo` of its own
    /// (core/src/structs.rs:59-62), so one batch may mix regex configs (`zke_verify_emails_mixed`).  The configs are the
    /// distinct id lists in order of first appearance; the capture tables are e-mail-major.  Result `i` is what
    /// `verify_emails_with_regex` gives input `i` in a batch of its own config.
    pub fn verify_emails_mixed(
        &self,
        inputs: &[EmailWithRegex],
    ) -> Result<Vec<Result<EmailWithRegexVerifierOutput, Panic>>, EngineError> {
        if inputs.is_empty() {
            return Ok(Vec::new());
        }
        let empty: Vec<CompiledRegex> = Vec::new();
        let ids = |engine: &Engine, parts: &Option<Vec<CompiledRegex>>| -> Result<Vec<u32>, EngineError> {
            let mut v = Vec::new();
            for p in parts.as_ref().unwrap_or(&empty) {
                let mut id = 0u32;
                // SAFETY: the slices outlive the call; the engine copies what it keeps.
                let rc = unsafe {
                    sys::zke_dfa_register(
                        engine.raw,
                        p.verify_re.fwd.as_ptr(),
                        p.verify_re.fwd.len(),
                        p.verify_re.bwd.as_ptr(),
                        p.verify_re.bwd.len(),
                        &mut id,
                    )
                };
                if rc != 0 {
                    return Err(engine.last_error(rc));
                }
                v.push(id);
            }
            Ok(v)
        };
        let mut lists: Vec<(Vec<u32>, Vec<u32>)> = Vec::new();
        let mut config_of: Vec<u32> = Vec::with_capacity(inputs.len());
        let mut cap_off: Vec<u32> = vec![0];
        let mut cap_str_off: Vec<u32> = vec![0];
        let mut cap_blob: Vec<u8> = Vec::new();
        for inp in inputs {
            let key = (ids(self, &inp.regex_info.header_parts)?, ids(self, &inp.regex_info.body_parts)?);
            let c = match lists.iter().position(|k| *k == key) {
                Some(c) => c,
                None => {
                    if lists.len() == sys::ZKE_MIXED_MAX_CONFIGS as usize {
                        return Err(EngineError { code: sys::ZKE_E_ARG, message: "more than ZKE_MIXED_MAX_CONFIGS regex configs in one batch; split it".into() });
                    }
                    lists.push(key);
                    lists.len() - 1
                }
            };
            config_of.push(c as u32);
            for parts in [&inp.regex_info.header_parts, &inp.regex_info.body_parts] {
                for p in parts.as_ref().unwrap_or(&empty) {
                    for s in p.captures.as_ref().map(|v| v.as_slice()).unwrap_or(&[]) {
                        cap_blob.extend_from_slice(s.as_bytes());
                        cap_str_off.push(cap_blob.len() as u32);
                    }
                    cap_off.push((cap_str_off.len() - 1) as u32);
                }
            }
        }
        if cap_blob.is_empty() {
            cap_blob.push(0);
        }
        let configs: Vec<sys::zke_regex_config> = lists
            .iter()
            .map(|(h, b)| sys::zke_regex_config {
                n_header_parts: h.len() as u32,
                header_part_ids: h.as_ptr(),
                n_body_parts: b.len() as u32,
                body_part_ids: b.as_ptr(),
            })
            .collect();
        let refs: Vec<sys::zke_email_ref> = inputs.iter().map(|i| email_ref(&i.email)).collect();
        let mixed = sys::zke_regex_mixed {
            n_configs: configs.len() as u32,
            configs: configs.as_ptr(),
            config_of: config_of.as_ptr(),
            cap_off: if cap_off.len() > 1 { cap_off.as_ptr() } else { ptr::null() },
            cap_str_off: cap_str_off.as_ptr(),
            cap_blob: cap_blob.as_ptr(),
        };
        let mut out = vec![zeroed_result(); inputs.len()];
        // SAFETY: as in verify_emails; the configs, their id lists and the capture tables live until the call returns.
        let rc = unsafe { sys::zke_verify_emails_mixed(self.raw, refs.as_ptr(), refs.len() as u32, &mixed, out.as_mut_ptr()) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(inputs
            .iter()
            .zip(out.iter())
            .map(|(inp, r)| {
                if r.status == sys::ZKE_OK {
                    Ok(EmailWithRegexVerifierOutput { email: email_output(&inp.email, r), regex_matches: regex_matches_of(&inp.regex_info) })
                } else {
                    Err(Panic { status: r.status, detail: r.detail })
                }
            })
            .collect())
    }

    /// One e-mail through the single-e-mail C entry point `zke_verify_email` (core/src/circuits.rs:9).
    pub fn try_verify_email(&self, email: &Email) -> Result<Result<EmailVerifierOutput, Panic>, EngineError> {
        let mut r = zeroed_result();
        let ext_null = email.external_inputs.iter().any(|x| x.value.is_none()) as u32;
        // SAFETY: the slices outlive the (synchronous) call; lengths are passed with them.
        let rc = unsafe {
            sys::zke_verify_email(
                self.raw,
                email.raw_email.as_ptr(),
                email.raw_email.len(),
                email.from_domain.as_ptr().cast(),
                email.from_domain.len(),
                email.public_key.key.as_ptr(),
                email.public_key.key.len(),
                key_type_code(&email.public_key.key_type) as u32,
                ext_null,
                &mut r,
            )
        };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(if r.status == sys::ZKE_OK { Ok(email_output(email, &r)) } else { Err(Panic { status: r.status, detail: r.detail }) })
    }

    /// One `EmailWithRegex` through `zke_verify_email_with_regex` (core/src/circuits.rs:31).
    pub fn try_verify_email_with_regex(
        &self,
        input: &EmailWithRegex,
    ) -> Result<Result<EmailWithRegexVerifierOutput, Panic>, EngineError> {
        // RegexInfo -> two zke_regex_part lists; the pointer tables live until the call returns
        struct Part {
            ptrs: Vec<*const u8>,
            lens: Vec<usize>,
        }
        let empty: Vec<CompiledRegex> = Vec::new();
        let mut keep: Vec<Part> = Vec::new();
        let mut lists: [Vec<sys::zke_regex_part>; 2] = [Vec::new(), Vec::new()];
        for (side, parts) in [&input.regex_info.header_parts, &input.regex_info.body_parts].into_iter().enumerate() {
            for p in parts.as_ref().unwrap_or(&empty) {
                let caps: &[String] = p.captures.as_ref().map(|v| v.as_slice()).unwrap_or(&[]);
                keep.push(Part { ptrs: caps.iter().map(|c| c.as_ptr()).collect(), lens: caps.iter().map(|c| c.len()).collect() });
                let k = keep.last().unwrap();
                lists[side].push(sys::zke_regex_part {
                    fwd: p.verify_re.fwd.as_ptr(),
                    fwd_len: p.verify_re.fwd.len(),
                    bwd: p.verify_re.bwd.as_ptr(),
                    bwd_len: p.verify_re.bwd.len(),
                    n_captures: caps.len() as u32,
                    captures: k.ptrs.as_ptr(),       // the Vec's heap buffer does not move when `keep` grows
                    capture_lens: k.lens.as_ptr(),
                });
            }
        }
        let email = &input.email;
        let mut r = zeroed_result();
        let ext_null = email.external_inputs.iter().any(|x| x.value.is_none()) as u32;
        // SAFETY: every pointer refers into `input`, `keep` or `lists`, all alive until the synchronous call returns.
        let rc = unsafe {
            sys::zke_verify_email_with_regex(
                self.raw,
                email.raw_email.as_ptr(),
                email.raw_email.len(),
                email.from_domain.as_ptr().cast(),
                email.from_domain.len(),
                email.public_key.key.as_ptr(),
                email.public_key.key.len(),
                key_type_code(&email.public_key.key_type) as u32,
                ext_null,
                lists[0].as_ptr(),
                lists[0].len() as u32,
                lists[1].as_ptr(),
                lists[1].len() as u32,
                &mut r,
            )
        };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(if r.status == sys::ZKE_OK {
            Ok(EmailWithRegexVerifierOutput { email: email_output(email, &r), regex_matches: regex_matches_of(&input.regex_info) })
        } else {
            Err(Panic { status: r.status, detail: r.detail })
        })
    }

    /// `helpers/src/generator.rs:17-30` for a slice (`zke_scan_signatures`): per e-mail `(status, detail, n_signatures,
    /// n_candidates)` and, for the first `max_sigs` DKIM-Signature headers, `validate_header`'s verdict (`code` 0: a candidate,
    /// `ZKE_D_NEUTRAL`: another domain's, else why it is refused), `a=` classified and the selector.
    pub fn scan_signatures(&self, raw_emails: &[&[u8]], from_domains: &[&str], max_sigs: u32) -> Result<Vec<SigScan>, EngineError> {
        if raw_emails.len() != from_domains.len() {
            return Err(EngineError { code: sys::ZKE_E_ARG, message: "one from_domain per raw e-mail".into() });
        }
        let n = raw_emails.len();
        let refs: Vec<sys::zke_email_ref> = raw_emails
            .iter()
            .zip(from_domains)
            .map(|(r, d)| sys::zke_email_ref {
                raw: r.as_ptr(),
                raw_len: r.len(),
                from_domain: d.as_ptr().cast(),
                domain_len: d.len(),
                key: ptr::null(),
                key_len: 0,
                key_type: 0,
                external_input_null: 0,
            })
            .collect();
        let mut status = vec![0u32; 4 * n + 1];
        let mut off = vec![0u32; n + 1];
        let zero = sys::zke_sig_info { header_index: 0, code: 0, algo: 0, sel_off: 0, sel_len: 0, val_start: 0, val_end: 0, reserved: 0 };
        let mut sigs = vec![zero; n * max_sigs as usize + 1];
        let mut blob = vec![0u8; n * max_sigs as usize * 32 + 1];
        for attempt in 0..2 {
            let mut o = sys::zke_sig_scan {
                scan_status: status.as_mut_ptr(),
                scan_status_cap: 4 * n,
                sig_off: off.as_mut_ptr(),
                sig_off_cap: n + 1,
                sigs: sigs.as_mut_ptr(),
                sigs_cap: n * max_sigs as usize,
                sel_blob: blob.as_mut_ptr(),
                sel_blob_cap: blob.len(),
                scan_status_need: 0,
                sig_off_need: 0,
                sigs_need: 0,
                sel_blob_need: 0,
                n_sigs: 0,
            };
            // SAFETY: every pointer refers into a Vec or slice that outlives the (synchronous) call, with its capacity beside it.
            let rc = unsafe { sys::zke_scan_signatures(self.raw, refs.as_ptr(), n as u32, max_sigs, &mut o) };
            if rc == sys::ZKE_E_NOMEM && attempt == 0 && o.sel_blob_need > blob.len() {
                blob.resize(o.sel_blob_need, 0); // the selectors need a larger blob: once more with the size the engine reports
                continue;
            }
            if rc != 0 {
                return Err(self.last_error(rc));
            }
            break;
        }
        Ok((0..n)
            .map(|i| SigScan {
                status: status[4 * i],
                detail: status[4 * i + 1],
                n_signatures: status[4 * i + 2],
                n_candidates: status[4 * i + 3],
                sigs: sigs[off[i] as usize..off[i + 1] as usize]
                    .iter()
                    .map(|s| SigInfo {
                        header_index: s.header_index,
                        code: s.code,
                        algo: s.algo,
                        selector: String::from_utf8_lossy(&blob[s.sel_off as usize..(s.sel_off + s.sel_len) as usize]).into_owned(),
                        value_span: (s.val_start, s.val_end),
                    })
                    .collect(),
            })
            .collect())
    }

    /// `helpers/src/generator.rs:31-45` for a slice (`zke_select_keys`): `candidate_keys[i]` are the keys fetched for e-mail i's
    /// candidates in the scan's order (`None`: the fetch failed).  Returns the records and, per e-mail, the first key under
    /// which it verifies (bit 31, `ZKE_SEL_AFTER_UNSUPPORTED`: an earlier candidate is outside what the engine implements) or
    /// `ZKE_SEL_NONE`.
    pub fn select_keys(
        &self,
        raw_emails: &[&[u8]],
        from_domains: &[&str],
        candidate_keys: &[Vec<Option<PublicKey>>],
    ) -> Result<(Vec<sys::zke_result>, Vec<u32>), EngineError> {
        let n = raw_emails.len();
        if from_domains.len() != n || candidate_keys.len() != n {
            return Err(EngineError { code: sys::ZKE_E_ARG, message: "one from_domain and one candidate list per raw e-mail".into() });
        }
        let refs: Vec<sys::zke_email_ref> = raw_emails
            .iter()
            .zip(from_domains)
            .map(|(r, d)| sys::zke_email_ref {
                raw: r.as_ptr(),
                raw_len: r.len(),
                from_domain: d.as_ptr().cast(),
                domain_len: d.len(),
                key: ptr::null(),
                key_len: 0,
                key_type: 0,
                external_input_null: 0,
            })
            .collect();
        let mut off: Vec<u32> = vec![0];
        let mut keys: Vec<sys::zke_key_ref> = Vec::new();
        for row in candidate_keys {
            for k in row {
                keys.push(match k {
                    Some(k) => sys::zke_key_ref { key: k.key.as_ptr(), key_len: k.key.len(), key_type: key_type_code(&k.key_type) as u32, reserved: 0 },
                    None => sys::zke_key_ref { key: ptr::null(), key_len: 0, key_type: 0, reserved: 0 },
                });
            }
            off.push(keys.len() as u32);
        }
        let mut out = vec![zeroed_result(); n];
        let mut chosen = vec![sys::ZKE_SEL_NONE; n];
        // SAFETY: every pointer refers into the arguments or the Vecs above, alive until the synchronous call returns.
        let rc = unsafe { sys::zke_select_keys(self.raw, refs.as_ptr(), n as u32, off.as_ptr(), keys.as_ptr(), out.as_mut_ptr(), chosen.as_mut_ptr()) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok((out, chosen))
    }

    /// `helpers/src/generator.rs:11-53 generate_email_inputs` for a slice, with the DNS fetch as the caller's closure:
    /// `fetch_key(from_domain, selector)` is called once per distinct pair, on the host, between the two GPU calls (`None`: the
    /// fetch failed).  One `Result` per e-mail: the `Email` carrying the first key under which it verifies, or what the
    /// reference's `Err` stands for — a `parse_mail` error (the scan's status), "No DKIM signatures found"
    /// (`ZKE_DKIM_NOT_PASS` / `ZKE_D_NO_SIGNATURE`), "No valid DKIM key found for any signature" (`ZKE_DKIM_NOT_PASS` with the
    /// last candidate's detail) — or `ZKE_UNSUPPORTED` where the engine cannot give the reference's answer.
    pub fn generate_email_inputs<F>(
        &self,
        from_domains: &[&str],
        raw_emails: &[&[u8]],
        mut fetch_key: F,
        external_inputs: Option<&[Vec<ExternalInput>]>,
    ) -> Result<Vec<Result<Email, Panic>>, EngineError>
    where
        F: FnMut(&str, &str) -> Option<PublicKey>,
    {
        let scans = self.scan_signatures(raw_emails, from_domains, sys::ZKE_SCAN_MAX_SIGS)?;
        let mut cache: std::collections::HashMap<(String, String), Option<PublicKey>> = std::collections::HashMap::new();
        let mut cands: Vec<Vec<Option<PublicKey>>> = Vec::with_capacity(scans.len());
        for (sc, dom) in scans.iter().zip(from_domains) {
            let mut row = Vec::new();
            for s in sc.sigs.iter().filter(|s| s.code == 0) {
                let key = (dom.to_string(), s.selector.clone());
                let k = cache.entry(key).or_insert_with(|| fetch_key(dom, &s.selector));
                row.push(k.clone());
            }
            cands.push(row);
        }
        let (recs, chosen) = self.select_keys(raw_emails, from_domains, &cands)?;
        Ok((0..scans.len())
            .map(|i| {
                let sc = &scans[i];
                if sc.status != sys::ZKE_OK {
                    return Err(Panic { status: sc.status, detail: sc.detail });
                }
                if sc.n_signatures == 0 {
                    return Err(Panic { status: sys::ZKE_DKIM_NOT_PASS, detail: sys::ZKE_D_NO_SIGNATURE }); // generator.rs:21
                }
                if chosen[i] == sys::ZKE_SEL_NONE {
                    if sc.n_candidates as usize > cands[i].len() {
                        return Err(Panic { status: sys::ZKE_UNSUPPORTED, detail: sys::ZKE_D_U_TOO_MANY_SIGS }); // the list was cut
                    }
                    let status = if recs[i].status == sys::ZKE_UNSUPPORTED { sys::ZKE_UNSUPPORTED } else { sys::ZKE_DKIM_NOT_PASS };
                    return Err(Panic { status, detail: recs[i].detail }); // generator.rs:52
                }
                if chosen[i] & sys::ZKE_SEL_AFTER_UNSUPPORTED != 0 {
                    return Err(Panic { status: sys::ZKE_UNSUPPORTED, detail: sys::ZKE_D_U_ALGO_ED25519 });
                }
                Ok(Email {
                    from_domain: from_domains[i].to_string(),
                    raw_email: raw_emails[i].to_vec(),
                    public_key: cands[i][chosen[i] as usize].clone().expect("a chosen candidate has a key"),
                    external_inputs: external_inputs.map(|x| x[i].clone()).unwrap_or_default(),
                })
            })
            .collect())
    }
}

/// The records of one call as `zke_keyrec_ref[m]` and the buffers of its `zke_keyrec_out` (3/4 of the records' bytes hold every key).
struct KeyrecCall {
    refs: Vec<sys::zke_keyrec_ref>,
    infos: Vec<sys::zke_key_info>,
    keys: Vec<u8>,
}

impl KeyrecCall {
    fn new(records: &[Option<&[u8]>]) -> Self {
        let refs: Vec<sys::zke_keyrec_ref> = records
            .iter()
            .map(|r| match r {
                Some(r) if !r.is_empty() => sys::zke_keyrec_ref { txt: r.as_ptr(), len: r.len() },
                _ => sys::zke_keyrec_ref { txt: ptr::null(), len: 0 },
            })
            .collect();
        let total: usize = refs.iter().map(|r| r.len).sum();
        let infos = vec![sys::zke_key_info { code: 0, key_type: 0, key_off: 0, key_len: 0 }; records.len() + 1];
        KeyrecCall { refs, infos, keys: vec![0u8; total * 3 / 4 + 1] }
    }

    fn out(&mut self) -> sys::zke_keyrec_out {
        sys::zke_keyrec_out {
            infos: self.infos.as_mut_ptr(),
            infos_cap: self.refs.len(),
            keys: self.keys.as_mut_ptr(),
            keys_cap: self.keys.len(),
            infos_need: 0,
            keys_need: 0,
        }
    }

    fn result(&self) -> Vec<KeyInfo> {
        self.infos[..self.refs.len()]
            .iter()
            .map(|f| KeyInfo { code: f.code, key_type: f.key_type, key: self.keys[f.key_off as usize..(f.key_off + f.key_len) as usize].to_vec() })
            .collect()
    }
}

impl Engine {
    /// `helpers/src/dkim.rs:67-111` for a slice (`zke_decode_key_records`): what a resolver returns -> the (key, key_type) pair of
    /// `Email.public_key`.  `mode`: `ZKE_KEYREC_DNS` (the TXT record of RFC 6376 3.6.1) or `ZKE_KEYREC_ARCHIVE` (the archive's value
    /// as dkim.rs reads it); `None` or an empty record: the fetch failed.
    pub fn decode_key_records(&self, records: &[Option<&[u8]>], mode: u32) -> Result<Vec<KeyInfo>, EngineError> {
        let mut call = KeyrecCall::new(records);
        let mut out = call.out();
        // SAFETY: every pointer refers into `records` or `call`, alive until the synchronous call returns.
        let rc = unsafe { sys::zke_decode_key_records(self.raw, call.refs.as_ptr(), call.refs.len() as u32, mode, &mut out) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(call.result())
    }

    /// `zke_select_keys_from_records`: `select_keys` with the resolver's raw answers in place of keys; the records are decoded on
    /// the GPU in front of the verify launches and the decoded keys stay in HBM on their way there.  Returns the records, `chosen`
    /// and, per e-mail, what each candidate decoded to.
    pub fn select_keys_from_records(
        &self,
        raw_emails: &[&[u8]],
        from_domains: &[&str],
        candidate_records: &[Vec<Option<Vec<u8>>>],
        mode: u32,
    ) -> Result<(Vec<sys::zke_result>, Vec<u32>, Vec<Vec<KeyInfo>>), EngineError> {
        let n = raw_emails.len();
        if from_domains.len() != n || candidate_records.len() != n {
            return Err(EngineError { code: sys::ZKE_E_ARG, message: "one from_domain and one candidate list per raw e-mail".into() });
        }
        let refs: Vec<sys::zke_email_ref> = raw_emails
            .iter()
            .zip(from_domains)
            .map(|(r, d)| sys::zke_email_ref {
                raw: r.as_ptr(),
                raw_len: r.len(),
                from_domain: d.as_ptr().cast(),
                domain_len: d.len(),
                key: ptr::null(),
                key_len: 0,
                key_type: 0,
                external_input_null: 0,
            })
            .collect();
        let mut off: Vec<u32> = vec![0];
        let mut flat: Vec<Option<&[u8]>> = Vec::new();
        for row in candidate_records {
            flat.extend(row.iter().map(|r| r.as_deref()));
            off.push(flat.len() as u32);
        }
        let mut call = KeyrecCall::new(&flat);
        let mut keys_out = call.out();
        let mut out = vec![zeroed_result(); n];
        let mut chosen = vec![sys::ZKE_SEL_NONE; n];
        // SAFETY: every pointer refers into the arguments, `call` or the Vecs above, alive until the synchronous call returns.
        let rc = unsafe {
            sys::zke_select_keys_from_records(self.raw, refs.as_ptr(), n as u32, off.as_ptr(), call.refs.as_ptr(), mode, out.as_mut_ptr(), chosen.as_mut_ptr(), &mut keys_out)
        };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        let all = call.result();
        let infos = (0..n).map(|i| all[off[i] as usize..off[i + 1] as usize].to_vec()).collect();
        Ok((out, chosen, infos))
    }

    /// `generate_email_inputs` with the resolver's RAW answers: `fetch_record(from_domain, selector)` returns the TXT record of
    /// `selector._domainkey.from_domain` (its character-strings joined) or the archive's value, `None` when the fetch failed.
    /// "Raw e-mails + the records in, `Email` values out": the caller is left with network code only.
    pub fn generate_email_inputs_from_records<F>(
        &self,
        from_domains: &[&str],
        raw_emails: &[&[u8]],
        mut fetch_record: F,
        mode: u32,
        external_inputs: Option<&[Vec<ExternalInput>]>,
    ) -> Result<Vec<Result<Email, Panic>>, EngineError>
    where
        F: FnMut(&str, &str) -> Option<Vec<u8>>,
    {
        let scans = self.scan_signatures(raw_emails, from_domains, sys::ZKE_SCAN_MAX_SIGS)?;
        let mut cache: std::collections::HashMap<(String, String), Option<Vec<u8>>> = std::collections::HashMap::new();
        let mut cands: Vec<Vec<Option<Vec<u8>>>> = Vec::with_capacity(scans.len());
        for (sc, dom) in scans.iter().zip(from_domains) {
            let mut row = Vec::new();
            for s in sc.sigs.iter().filter(|s| s.code == 0) {
                let key = (dom.to_string(), s.selector.clone());
                let k = cache.entry(key).or_insert_with(|| fetch_record(dom, &s.selector));
                row.push(k.clone());
            }
            cands.push(row);
        }
        let (recs, chosen, infos) = self.select_keys_from_records(raw_emails, from_domains, &cands, mode)?;
        Ok((0..scans.len())
            .map(|i| {
                let sc = &scans[i];
                if sc.status != sys::ZKE_OK {
                    return Err(Panic { status: sc.status, detail: sc.detail });
                }
                if sc.n_signatures == 0 {
                    return Err(Panic { status: sys::ZKE_DKIM_NOT_PASS, detail: sys::ZKE_D_NO_SIGNATURE }); // generator.rs:21
                }
                if chosen[i] == sys::ZKE_SEL_NONE {
                    if sc.n_candidates as usize > cands[i].len() {
                        return Err(Panic { status: sys::ZKE_UNSUPPORTED, detail: sys::ZKE_D_U_TOO_MANY_SIGS }); // the list was cut
                    }
                    let status = if recs[i].status == sys::ZKE_UNSUPPORTED { sys::ZKE_UNSUPPORTED } else { sys::ZKE_DKIM_NOT_PASS };
                    return Err(Panic { status, detail: recs[i].detail }); // generator.rs:52
                }
                if chosen[i] & sys::ZKE_SEL_AFTER_UNSUPPORTED != 0 {
                    return Err(Panic { status: sys::ZKE_UNSUPPORTED, detail: sys::ZKE_D_U_ALGO_ED25519 });
                }
                Ok(Email {
                    from_domain: from_domains[i].to_string(),
                    raw_email: raw_emails[i].to_vec(),
                    public_key: infos[i][chosen[i] as usize].public_key(),
                    external_inputs: external_inputs.map(|x| x[i].clone()).unwrap_or_default(),
                })
            })
            .collect())
    }
}

/// One part of a capture extraction (`zke_capture_part`): the registered DFA pair that finds the match, the registered capture
/// program of the same pattern, the groups wanted (`RegexPattern.capture_indices`).
#[derive(Clone, Debug)]
pub struct CapturePart {
    pub dfa_id: u32,
    pub prog_id: u32,
    pub groups: Vec<u32>,
}

/// What `extract_captures_mapped` delivers: the records, the tables of `zke_capture_out` and the origins of `zke_capture_origin`.
/// `spans` / `origin_spans`: `{start, end}` per (e-mail, requested group) in the part's haystack and in the haystack BEFORE the QP
/// filter (the canonical body as it was signed); `origin_flags`: `ZKE_ORGF_SPLIT` / `ZKE_ORGF_PADDING`.
#[derive(Clone)]
pub struct MappedCaptures {
    pub records: Vec<sys::zke_result>,
    pub spans: Vec<u32>,
    pub flags: Vec<u8>,
    pub cap_off: Vec<u32>,
    pub cap_str_off: Vec<u32>,
    pub cap_blob: Vec<u8>,
    pub origin_spans: Vec<u32>,
    pub origin_flags: Vec<u8>,
}

/// One e-mail's verifier output as a batch encodes it on the device (`zke_encoded_info`, the encoding as bytes):
/// `VerificationOutput::from_parts(email, None).abi_encode()` (`core/src/io.rs:28-44`) — what a zkVM front end commits as public
/// values — and the SHA-256 of those bytes, the value a proof binds to.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct EncodedOutput {
    pub bytes: Vec<u8>,
    pub digest: [u8; 32],
}

impl Engine {
    /// `verify_email` over a slice with the outputs encoded and hashed on the device (`zke_verify_emails_encoded`, both list forms
    /// NULL): one `Result` per e-mail, in order — the encoding and its digest, or the panic the reference would have raised.  The
    /// external inputs travel flattened `[name1, value1, ...]` as `circuits.rs:18-27` flattens them; a `None` value travels as `""`
    /// (its e-mail reports `ZKE_EXTERNAL_INPUT_NULL` and is not encoded).  Both buffer sizes follow from the inputs' lengths alone:
    /// a first call that stages nothing asks for them, the second runs the batch.
    pub fn verify_emails_encoded(&self, emails: &[Email]) -> Result<Vec<Result<EncodedOutput, Panic>>, EngineError> {
        let n = emails.len();
        if n == 0 {
            return Ok(Vec::new());
        }
        let refs: Vec<sys::zke_email_ref> = emails.iter().map(email_ref).collect();
        let (mut ext_off, mut ext_str_off, mut ext_blob) = (vec![0u32], vec![0u32], Vec::<u8>::new());
        for e in emails {
            for x in &e.external_inputs {
                ext_blob.extend_from_slice(x.name.as_bytes());
                ext_str_off.push(ext_blob.len() as u32);
                ext_blob.extend_from_slice(x.value.as_deref().unwrap_or("").as_bytes());
                ext_str_off.push(ext_blob.len() as u32);
            }
            ext_off.push(ext_str_off.len() as u32 - 1);
        }
        ext_blob.push(0); // (a valid pointer also when every string is empty)
        let input = sys::zke_encode_in {
            lists: ptr::null(),
            mixed: ptr::null(),
            ext_off: ext_off.as_ptr(),
            ext_str_off: ext_str_off.as_ptr(),
            ext_blob: ext_blob.as_ptr(),
        };
        let mut out = vec![zeroed_result(); n];
        let mut enc = sys::zke_encoded_out { infos: ptr::null_mut(), infos_cap: 0, bytes: ptr::null_mut(), bytes_cap: 0, infos_need: 0, bytes_need: 0 };
        // SAFETY: every pointer refers into `emails`, `refs`, the three tables or `out`, alive until the synchronous call returns;
        // with zero capacities the call writes the two sizes and returns ZKE_E_NOMEM before anything is staged.
        let rc = unsafe { sys::zke_verify_emails_encoded(self.raw, refs.as_ptr(), n as u32, &input, out.as_mut_ptr(), &mut enc) };
        if rc != sys::ZKE_E_NOMEM {
            return Err(self.last_error(if rc == 0 { sys::ZKE_E_ARG } else { rc }));
        }
        // SAFETY: zke_encoded_info is plain integers and bytes; all-zero is a value of it.
        let mut infos: Vec<sys::zke_encoded_info> = vec![unsafe { std::mem::zeroed() }; enc.infos_need];
        let mut bytes = vec![0u8; enc.bytes_need];
        enc = sys::zke_encoded_out { infos: infos.as_mut_ptr(), infos_cap: infos.len(), bytes: bytes.as_mut_ptr(), bytes_cap: bytes.len(), infos_need: 0, bytes_need: 0 };
        // SAFETY: as above; `infos` and `bytes` have exactly the sizes the first call asked for.
        let rc = unsafe { sys::zke_verify_emails_encoded(self.raw, refs.as_ptr(), n as u32, &input, out.as_mut_ptr(), &mut enc) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(out
            .iter()
            .zip(infos.iter())
            .map(|(r, f)| {
                if r.status == sys::ZKE_OK {
                    Ok(EncodedOutput { bytes: bytes[f.off as usize..f.off as usize + f.len as usize].to_vec(), digest: f.digest })
                } else {
                    Err(Panic { status: r.status, detail: r.detail })
                }
            })
            .collect())
    }
}

/// One e-mail's `extract_email_body` as an extraction reports it (`zke_body_info`, the decoded body as bytes).
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct BodyInfo {
    /// `ZKE_OK` | `ZKE_PARSE_FAIL` | `ZKE_BODY_DECODE_FAIL` | `ZKE_UNSUPPORTED`, and the rule or limit it names.
    pub status: u32,
    pub detail: u32,
    /// 0: the message itself; k >= 1: its k-th direct subpart; bit 31: chosen as text/html.
    pub part: u32,
    /// `ZKE_CTE_*`.
    pub encoding: u32,
    /// `body_bytes` of the chosen part inside the raw e-mail, before decoding.
    pub src_span: (u32, u32),
    /// Empty unless `status` is `ZKE_OK`.
    pub body: Vec<u8>,
}

impl Engine {
    /// `extract_email_body(&parse_mail(raw).unwrap())` (`core/src/email.rs:7-23`) over a slice of raw e-mails (`zke_extract_bodies`):
    /// the text/html subpart (else the first, else the message) with its Content-Transfer-Encoding undone.  `part_keeps_eol`:
    /// `ZKE_BODYF_PART_KEEPS_EOL`, the line break in front of a boundary line stays part of the body.
    pub fn extract_email_bodies(&self, raw_emails: &[&[u8]], part_keeps_eol: bool) -> Result<Vec<BodyInfo>, EngineError> {
        let n = raw_emails.len();
        let refs: Vec<sys::zke_email_ref> = raw_emails
            .iter()
            .map(|r| sys::zke_email_ref {
                raw: r.as_ptr(),
                raw_len: r.len(),
                from_domain: ptr::null(),
                domain_len: 0,
                key: ptr::null(),
                key_len: 0,
                key_type: 0,
                external_input_null: 0,
            })
            .collect();
        let total: usize = raw_emails.iter().map(|r| r.len()).sum();
        // SAFETY: zke_body_info is plain integers; all-zero is a value of it.
        let mut infos: Vec<sys::zke_body_info> = vec![unsafe { std::mem::zeroed() }; n];
        let mut bytes = vec![0u8; 2 * total + 1];      // a decoded body is at most twice its source (lone LF becomes CRLF)
        let mut out = sys::zke_body_out {
            infos: infos.as_mut_ptr(),
            infos_cap: n,
            bytes: bytes.as_mut_ptr(),
            bytes_cap: bytes.len(),
            infos_need: 0,
            bytes_need: 0,
        };
        let flags = if part_keeps_eol { sys::ZKE_BODYF_PART_KEEPS_EOL } else { 0 };
        // SAFETY: every pointer refers into `raw_emails`, `refs`, `infos` or `bytes`, alive until the synchronous call returns.
        let rc = unsafe { sys::zke_extract_bodies(self.raw, refs.as_ptr(), n as u32, flags, &mut out) };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok(infos
            .iter()
            .map(|f| BodyInfo {
                status: f.status,
                detail: f.detail,
                part: f.part,
                encoding: f.encoding,
                src_span: (f.src_off, f.src_off + f.src_len),
                body: bytes[f.body_off as usize..f.body_off as usize + f.body_len as usize].to_vec(),
            })
            .collect())
    }

    /// `remove_quoted_printable_soft_breaks` (`core/src/email.rs:61-86`) over a slice of bodies (`zke_qp_clean_batch`), both return
    /// values per body: the body without its soft breaks, zero-padded to its length, and `index_map` with `usize::MAX` over the padding.
    pub fn remove_quoted_printable_soft_breaks_batch(&self, bodies: &[&[u8]]) -> Result<Vec<(Vec<u8>, Vec<usize>)>, EngineError> {
        let mut off: Vec<u64> = vec![0];
        let mut blob: Vec<u8> = Vec::new();
        for b in bodies {
            blob.extend_from_slice(b);
            off.push(blob.len() as u64);
        }
        let mut cleaned = vec![0u8; blob.len()];
        let mut map = vec![0u32; blob.len()];
        let mut kept = vec![0u32; bodies.len()];
        // SAFETY: the three outputs hold off[n] bytes / entries and n entries; every pointer is alive until the synchronous call returns.
        let rc = unsafe {
            sys::zke_qp_clean_batch(self.raw, blob.as_ptr(), off.as_ptr(), bodies.len() as u32, cleaned.as_mut_ptr(), map.as_mut_ptr(), kept.as_mut_ptr())
        };
        if rc != 0 {
            return Err(self.last_error(rc));
        }
        Ok((0..bodies.len())
            .map(|i| {
                let (a, b) = (off[i] as usize, off[i + 1] as usize);
                (cleaned[a..b].to_vec(), map[a..b].iter().map(|&x| if x == sys::ZKE_QP_NO_INDEX { usize::MAX } else { x as usize }).collect())
            })
            .collect())
    }

    /// `String::from_utf8_lossy` (`helpers/src/regex.rs:35`) over a slice of byte strings on the device (`zke_utf8_lossy_batch`): per
    /// string the repaired text — every ill-formed chunk one U+FFFD — and whether it was changed.
    pub fn utf8_lossy_batch(&self, strings: &[&[u8]]) -> Result<Vec<(String, bool)>, EngineError> {
        let mut off: Vec<u64> = vec![0];
        let mut blob: Vec<u8> = Vec::new();
        for s in strings {
            blob.extend_from_slice(s);
            off.push(blob.len() as u64);
        }
        let n = strings.len();
        let mut out_off = vec![0u32; n + 1];
        let mut flags = vec![0u8; n + 1];
        let mut out = vec![0u8; blob.len() + blob.len() / 8 + 64];
        let mut need: usize = 0;
        for _attempt in 0..2 {
            // SAFETY: out_off holds n + 1 entries, flags n, out its length; every pointer is alive until the synchronous call returns.
            let rc = unsafe {
                sys::zke_utf8_lossy_batch(self.raw, blob.as_ptr(), off.as_ptr(), n as u32, out_off.as_mut_ptr(), out.as_mut_ptr(), out.len(), &mut need, flags.as_mut_ptr())
            };
            if rc == sys::ZKE_E_NOMEM && need > out.len() {
                out = vec![0u8; need];      // the repaired strings need a larger blob: once more with the size the engine reports
                continue;
            }
            if rc != 0 {
                return Err(self.last_error(rc));
            }
            break;
        }
        Ok((0..n)
            .map(|i| (String::from_utf8_lossy(&out[out_off[i] as usize..out_off[i + 1] as usize]).into_owned(), flags[i] & 1 != 0))
            .collect())
    }

    /// `zke_extract_captures_encoded`: from raw e-mails, keys and a part list to the public values in ONE batch — verify_email, the
    /// extraction, `String::from_utf8_lossy`, `abi_encode` and SHA-256 on the device.  Returns the tables (the strings of `cap_blob`
    /// are the REPAIRED strings, `CompiledRegex.captures` as the reference holds them; the origins are empty) and one `Result` per
    /// e-mail: the encoding of its `EmailWithRegexVerifierOutput` and the digest, or the panic the reference would have raised.
    /// One call when the first guess of the two variable-size buffers holds, else a second with the exact needs.
    pub fn extract_captures_encoded(
        &self,
        emails: &[Email],
        header_parts: &[CapturePart],
        body_parts: &[CapturePart],
    ) -> Result<(MappedCaptures, Vec<Result<EncodedOutput, Panic>>), EngineError> {
        let n = emails.len();
        let refs: Vec<sys::zke_email_ref> = emails.iter().map(email_ref).collect();
        let part = |p: &CapturePart| sys::zke_capture_part { dfa_id: p.dfa_id, prog_id: p.prog_id, n_groups: p.groups.len() as u32, groups: p.groups.as_ptr() };
        let hp: Vec<sys::zke_capture_part> = header_parts.iter().map(part).collect();
        let bp: Vec<sys::zke_capture_part> = body_parts.iter().map(part).collect();
        let g: usize = header_parts.iter().chain(body_parts).map(|p| p.groups.len()).sum();
        let (np, ng) = (n * (hp.len() + bp.len()), n * g);
        let (mut ext_off, mut ext_str_off, mut ext_blob) = (vec![0u32], vec![0u32], Vec::<u8>::new());
        for e in emails {
            for x in &e.external_inputs {
                ext_blob.extend_from_slice(x.name.as_bytes());
                ext_str_off.push(ext_blob.len() as u32);
                ext_blob.extend_from_slice(x.value.as_deref().unwrap_or("").as_bytes());
                ext_str_off.push(ext_blob.len() as u32);
            }
            ext_off.push(ext_str_off.len() as u32 - 1);
        }
        ext_blob.push(0); // (a valid pointer also when every string is empty)
        let mut m = MappedCaptures {
            records: vec![zeroed_result(); n],
            spans: vec![0; ng * 2],
            flags: vec![0; ng],
            cap_off: vec![0; np + 1],
            cap_str_off: vec![0; ng + 1],
            cap_blob: vec![0; ng * 64 + 1],
            origin_spans: Vec::new(),
            origin_flags: Vec::new(),
        };
        // SAFETY: zke_encoded_info is plain integers and bytes; all-zero is a value of it.
        let mut infos: Vec<sys::zke_encoded_info> = vec![unsafe { std::mem::zeroed() }; n];
        let mut bytes = vec![0u8; n * 512 + 2 * ext_blob.len() + 64 * ext_str_off.len() + ng * 160 + 1];
        for attempt in 0..2 {
            let mut caps: sys::zke_capture_out = unsafe { std::mem::zeroed() };
            caps.spans = m.spans.as_mut_ptr();
            caps.spans_cap = ng * 2;
            caps.flags = m.flags.as_mut_ptr();
            caps.flags_cap = ng;
            caps.cap_off = m.cap_off.as_mut_ptr();
            caps.cap_off_cap = np + 1;
            caps.cap_str_off = m.cap_str_off.as_mut_ptr();
            caps.cap_str_off_cap = ng + 1;
            caps.cap_blob = m.cap_blob.as_mut_ptr();
            caps.cap_blob_cap = m.cap_blob.len();
            let mut enc = sys::zke_encoded_out { infos: infos.as_mut_ptr(), infos_cap: n, bytes: bytes.as_mut_ptr(), bytes_cap: bytes.len(), infos_need: 0, bytes_need: 0 };
            // SAFETY: every pointer refers into the arguments, the tables, `m`, `infos` or `bytes`, alive and unmoved until the synchronous call returns.
            let rc = unsafe {
                sys::zke_extract_captures_encoded(self.raw, refs.as_ptr(), n as u32, hp.as_ptr(), hp.len() as u32, bp.as_ptr(), bp.len() as u32, m.records.as_mut_ptr(), &mut caps, ext_off.as_ptr(), ext_str_off.as_ptr(), ext_blob.as_ptr(), &mut enc)
            };
            if rc == sys::ZKE_E_NOMEM && attempt == 0 {
                // the needs are exact: once more with the sizes the engine reports
                if caps.cap_blob_need > m.cap_blob.len() {
                    m.cap_blob = vec![0; caps.cap_blob_need];
                }
                if enc.bytes_need > bytes.len() {
                    bytes = vec![0; enc.bytes_need];
                }
                continue;
            }
            if rc != 0 {
                return Err(self.last_error(rc));
            }
            m.cap_str_off.truncate(caps.n_strings + 1);
            m.cap_blob.truncate(caps.cap_blob_need);
            break;
        }
        let outs = m
            .records
            .iter()
            .zip(infos.iter())
            .map(|(r, f)| {
                if r.status == sys::ZKE_OK {
                    Ok(EncodedOutput { bytes: bytes[f.off as usize..f.off as usize + f.len as usize].to_vec(), digest: f.digest })
                } else {
                    Err(Panic { status: r.status, detail: r.detail })
                }
            })
            .collect();
        Ok((m, outs))
    }

    /// `zke_extract_captures_mapped` over a slice of e-mails that share one part list: verify_email, canonicalise, QP clean, exactly
    /// one match per part, the requested groups — and where each of them lies in the body as it was signed.
    pub fn extract_captures_mapped(&self, emails: &[Email], header_parts: &[CapturePart], body_parts: &[CapturePart]) -> Result<MappedCaptures, EngineError> {
        let n = emails.len();
        let refs: Vec<sys::zke_email_ref> = emails.iter().map(email_ref).collect();
        let part = |p: &CapturePart| sys::zke_capture_part { dfa_id: p.dfa_id, prog_id: p.prog_id, n_groups: p.groups.len() as u32, groups: p.groups.as_ptr() };
        let hp: Vec<sys::zke_capture_part> = header_parts.iter().map(part).collect();
        let bp: Vec<sys::zke_capture_part> = body_parts.iter().map(part).collect();
        let g: usize = header_parts.iter().chain(body_parts).map(|p| p.groups.len()).sum();
        let (np, ng) = (n * (hp.len() + bp.len()), n * g);
        let mut m = MappedCaptures {
            records: vec![zeroed_result(); n],
            spans: vec![0; ng * 2],
            flags: vec![0; ng],
            cap_off: vec![0; np + 1],
            cap_str_off: vec![0; ng + 1],
            cap_blob: vec![0; ng * 32 + 1],
            origin_spans: vec![0; ng * 2],
            origin_flags: vec![0; ng],
        };
        for attempt in 0..2 {
            let mut caps: sys::zke_capture_out = unsafe { std::mem::zeroed() };
            caps.spans = m.spans.as_mut_ptr();
            caps.spans_cap = ng * 2;
            caps.flags = m.flags.as_mut_ptr();
            caps.flags_cap = ng;
            caps.cap_off = m.cap_off.as_mut_ptr();
            caps.cap_off_cap = np + 1;
            caps.cap_str_off = m.cap_str_off.as_mut_ptr();
            caps.cap_str_off_cap = ng + 1;
            caps.cap_blob = m.cap_blob.as_mut_ptr();
            caps.cap_blob_cap = m.cap_blob.len();
            let mut org: sys::zke_capture_origin = unsafe { std::mem::zeroed() };
            org.spans = m.origin_spans.as_mut_ptr();
            org.spans_cap = ng * 2;
            org.flags = m.origin_flags.as_mut_ptr();
            org.flags_cap = ng;
            // SAFETY: every pointer refers into the arguments or `m`, alive and unmoved until the synchronous call returns.
            let rc = unsafe {
                sys::zke_extract_captures_mapped(self.raw, refs.as_ptr(), n as u32, hp.as_ptr(), hp.len() as u32, bp.as_ptr(), bp.len() as u32, m.records.as_mut_ptr(), &mut caps, &mut org)
            };
            if rc == sys::ZKE_E_NOMEM && attempt == 0 && caps.cap_blob_need > m.cap_blob.len() {
                m.cap_blob = vec![0; caps.cap_blob_need];      // the strings need a larger blob: once more with the size the engine reports
                continue;
            }
            if rc != 0 {
                return Err(self.last_error(rc));
            }
            m.cap_str_off.truncate(caps.n_strings + 1);
            m.cap_blob.truncate(caps.cap_blob_need);
            break;
        }
        Ok(m)
    }

    /// `zke_extract_captures_mixed`: the extraction over e-mails that carry different regex configs, in ONE batch.  `configs`: the
    /// distinct configs (header parts, body parts); `config_of[i]`: e-mail i's, or `ZKE_CONFIG_NONE` (verify_email only).  The tables
    /// are ragged — `cap_off` has J + 1 entries, spans / flags / origins are indexed by column (the header's job_off / col_off) —
    /// and `cap_off` / `cap_str_off` / `cap_blob` are what `verify_emails_mixed`'s C entry takes.
    pub fn extract_captures_mixed(&self, emails: &[Email], configs: &[(Vec<CapturePart>, Vec<CapturePart>)], config_of: &[u32]) -> Result<MappedCaptures, EngineError> {
        let n = emails.len();
        assert_eq!(config_of.len(), n, "one config index (or ZKE_CONFIG_NONE) per e-mail");
        let refs: Vec<sys::zke_email_ref> = emails.iter().map(email_ref).collect();
        let part = |p: &CapturePart| sys::zke_capture_part { dfa_id: p.dfa_id, prog_id: p.prog_id, n_groups: p.groups.len() as u32, groups: p.groups.as_ptr() };
        let parts: Vec<Vec<sys::zke_capture_part>> = configs.iter().map(|(h, b)| h.iter().chain(b).map(part).collect()).collect();
        let cfgs: Vec<sys::zke_capture_config> = configs
            .iter()
            .zip(&parts)
            .map(|((h, b), p)| sys::zke_capture_config {
                n_header_parts: h.len() as u32,
                header_parts: p.as_ptr(),
                n_body_parts: b.len() as u32,
                body_parts: p[h.len()..].as_ptr(),
            })
            .collect();
        let groups: Vec<usize> = configs.iter().map(|(h, b)| h.iter().chain(b).map(|p| p.groups.len()).sum()).collect();
        let (mut nj, mut ng) = (0usize, 0usize);
        for &c in config_of {
            if c != sys::ZKE_CONFIG_NONE {
                let c = c as usize;
                assert!(c < configs.len(), "config_of names no config");
                nj += parts[c].len();
                ng += groups[c];
            }
        }
        let mixed = sys::zke_capture_mixed { n_configs: cfgs.len() as u32, configs: cfgs.as_ptr(), config_of: config_of.as_ptr() };
        let mut m = MappedCaptures {
            records: vec![zeroed_result(); n],
            spans: vec![0; ng * 2],
            flags: vec![0; ng],
            cap_off: vec![0; nj + 1],
            cap_str_off: vec![0; ng + 1],
            cap_blob: vec![0; ng * 32 + 1],
            origin_spans: vec![0; ng * 2],
            origin_flags: vec![0; ng],
        };
        for attempt in 0..2 {
            let mut caps: sys::zke_capture_out = unsafe { std::mem::zeroed() };
            caps.spans = m.spans.as_mut_ptr();
            caps.spans_cap = ng * 2;
            caps.flags = m.flags.as_mut_ptr();
            caps.flags_cap = ng;
            caps.cap_off = m.cap_off.as_mut_ptr();
            caps.cap_off_cap = nj + 1;
            caps.cap_str_off = m.cap_str_off.as_mut_ptr();
            caps.cap_str_off_cap = ng + 1;
            caps.cap_blob = m.cap_blob.as_mut_ptr();
            caps.cap_blob_cap = m.cap_blob.len();
            let mut org: sys::zke_capture_origin = unsafe { std::mem::zeroed() };
            org.spans = m.origin_spans.as_mut_ptr();
            org.spans_cap = ng * 2;
            org.flags = m.origin_flags.as_mut_ptr();
            org.flags_cap = ng;
            // SAFETY: every pointer refers into the arguments, `parts`, `cfgs` or `m`, alive and unmoved until the synchronous call returns.
            let rc = unsafe { sys::zke_extract_captures_mixed(self.raw, refs.as_ptr(), n as u32, &mixed, m.records.as_mut_ptr(), &mut caps, &mut org) };
            if rc == sys::ZKE_E_NOMEM && attempt == 0 && caps.cap_blob_need > m.cap_blob.len() {
                m.cap_blob = vec![0; caps.cap_blob_need];
                continue;
            }
            if rc != 0 {
                return Err(self.last_error(rc));
            }
            m.cap_str_off.truncate(caps.n_strings + 1);
            m.cap_blob.truncate(caps.cap_blob_need);
            break;
        }
        Ok(m)
    }
}

impl Drop for Engine {
    fn drop(&mut self) {
        // SAFETY: the handle came from zke_engine_create and is destroyed once.
        unsafe { sys::zke_engine_destroy(self.raw) };
    }
}

/// The process-wide engine behind the two free functions (device: the current HIP device).
/// Shared without a lock: the C-ABI's entry points are re-entrant (one submission slot per call in flight).
pub fn default_engine() -> &'static Engine {
    static ENGINE: OnceLock<Engine> = OnceLock::new();
    ENGINE.get_or_init(|| Engine::new(-1).expect("zkemail_amd: no usable GPU engine (there is no CPU fallback)"))
}

/// `zkemail_core::verify_email` (core/src/circuits.rs:9-29): same signature, same panics.
pub fn verify_email(email: &Email) -> EmailVerifierOutput {
    match default_engine().try_verify_email(email) {
        Err(e) => panic!("{e}"),
        Ok(Err(p)) => panic!("{p}"),
        Ok(Ok(out)) => out,
    }
}

/// `zkemail_helpers::generate_email_inputs` (helpers/src/generator.rs:11-53) with the key fetch as a closure instead of the
/// reference's DNS lookup: `Err` where the reference returns `Err`.
pub fn generate_email_inputs<F>(
    from_domain: &str,
    raw_email: &[u8],
    fetch_key: F,
    external_inputs: Option<Vec<ExternalInput>>,
) -> Result<Email, Panic>
where
    F: FnMut(&str, &str) -> Option<PublicKey>,
{
    let ext = [external_inputs.unwrap_or_default()];
    match default_engine().generate_email_inputs(&[from_domain], &[raw_email], fetch_key, Some(&ext)) {
        Err(e) => panic!("{e}"),
        Ok(mut v) => v.remove(0),
    }
}

/// `generate_email_inputs` with the resolver's raw answer (TXT record or archive value) in place of the key: what
/// `helpers/src/dkim.rs:67-111` does with it runs on the GPU.
pub fn generate_email_inputs_from_records<F>(
    from_domain: &str,
    raw_email: &[u8],
    fetch_record: F,
    mode: u32,
    external_inputs: Option<Vec<ExternalInput>>,
) -> Result<Email, Panic>
where
    F: FnMut(&str, &str) -> Option<Vec<u8>>,
{
    let ext = [external_inputs.unwrap_or_default()];
    match default_engine().generate_email_inputs_from_records(&[from_domain], &[raw_email], fetch_record, mode, Some(&ext)) {
        Err(e) => panic!("{e}"),
        Ok(mut v) => v.remove(0),
    }
}

/// `zkemail_core::verify_email_with_regex` (core/src/circuits.rs:31-68): same signature, same panics.
pub fn verify_email_with_regex(input: &EmailWithRegex) -> EmailWithRegexVerifierOutput {
    match default_engine().try_verify_email_with_regex(input) {
        Err(e) => panic!("{e}"),
        Ok(Err(p)) => panic!("{p}"),
        Ok(Ok(out)) => out,
    }
}

/// `zkemail_core::extract_email_body` (core/src/email.rs:7-23) over the raw e-mail — `extract_email_body(&parse_mail(raw).unwrap())`:
/// the decoded body of the text/html subpart (else the first subpart, else the message).  Panics where the reference panics
/// (`email.rs:26` the parse, `email.rs:17-21` get_body_raw) and for an input the engine does not decide.
pub fn extract_email_body(raw: &[u8]) -> Vec<u8> {
    match default_engine().extract_email_bodies(&[raw], false) {
        Err(e) => panic!("{e}"),
        Ok(mut v) => {
            let f = v.remove(0);
            if f.status != sys::ZKE_OK {
                panic!("{}", Panic { status: f.status, detail: f.detail });
            }
            f.body
        }
    }
}
