#!/usr/bin/env python3
"""Generate the throw-away RSA test keys in tests/golden/keys.json with the openssl CLI.

Run once in the build container (`python tools/gen_keys.py`); the JSON is committed so the
GPU box and later rounds never need openssl.  Keys already in the file are kept as they are: only
names of the plan that are missing are generated, so the plan grows without changing the workloads' keys.
Public keys are stored as PKCS#1 ``RSAPublicKey`` DER — the form helpers/src/dkim.rs:50,96-102 hands to zkemail_core — as
written by ``openssl rsa -RSAPublicKey_out -outform DER`` (not by our own encoder).
"""
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "keys.json")


def der_items(b, pos):
    """Parse one DER TLV at pos -> (tag, value, next)."""
    tag = b[pos]
    ln = b[pos + 1]
    pos += 2
    if ln & 0x80:
        k = ln & 0x7F
        ln = int.from_bytes(b[pos:pos + k], "big")
        pos += k
    return tag, b[pos:pos + ln], pos + ln


def der_int(x):
    b = x.to_bytes(x.bit_length() // 8 + 1, "big")                # minimal, with a leading 0 when the top bit is set
    return der_tlv(0x02, b[1:] if len(b) > 1 and b[0] == 0 and not b[1] & 0x80 else b)


def der_tlv(tag, v):
    n = len(v)
    ln = bytes([n]) if n < 0x80 else bytes([0x80 | ((n.bit_length() + 7) // 8)]) + n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([tag]) + ln + v


def exact_private_der(bits, e):
    """openssl genpkey makes 2049-, 3071- and 4095-bit requests one or two bits short: two primes from `openssl prime`
    whose product has exactly `bits` bits, as a PKCS#1 RSAPrivateKey for openssl to check and to write out."""
    def prime(b):
        return int(subprocess.run(["openssl", "prime", "-generate", "-bits", str(b)], check=True, capture_output=True,
                                  text=True).stdout)
    while True:
        p, q = prime((bits + 1) // 2), prime(bits // 2)
        n, phi = p * q, (p - 1) * (q - 1)
        if p != q and n.bit_length() == bits and math.gcd(e, phi) == 1:
            break
    d = pow(e, -1, math.lcm(p - 1, q - 1))
    body = b"".join(der_int(x) for x in (0, n, e, d, p, q, d % (p - 1), d % (q - 1), pow(q, -1, p)))
    return der_tlv(0x30, body)


def gen(bits, e=65537):
    with tempfile.TemporaryDirectory() as td:
        priv = os.path.join(td, "k.pem")
        subprocess.run(["openssl", "genpkey", "-algorithm", "RSA", "-pkeyopt", f"rsa_keygen_bits:{bits}",
                        "-pkeyopt", f"rsa_keygen_pubexp:{e}", "-out", priv], check=True, capture_output=True)
        der = subprocess.run(["openssl", "rsa", "-in", priv, "-traditional", "-outform", "DER"],
                             check=True, capture_output=True).stdout
        tag, seq, _ = der_items(der, 0)
        if int.from_bytes(der_items(seq, der_items(seq, 0)[2])[1], "big").bit_length() != bits:
            priv = os.path.join(td, "k.der")
            with open(priv, "wb") as f:
                f.write(exact_private_der(bits, e))
            subprocess.run(["openssl", "rsa", "-inform", "DER", "-in", priv, "-check", "-noout"], check=True, capture_output=True)
            der = subprocess.run(["openssl", "rsa", "-inform", "DER", "-in", priv, "-traditional", "-outform", "DER"],
                                 check=True, capture_output=True).stdout
        pub = subprocess.run(["openssl", "rsa", "-in", priv, "-RSAPublicKey_out", "-outform", "DER"] +
                             (["-inform", "DER"] if priv.endswith(".der") else []), check=True, capture_output=True).stdout
    tag, seq, _ = der_items(der, 0)
    assert tag == 0x30
    vals, pos = [], 0
    while pos < len(seq):
        t, v, pos = der_items(seq, pos)
        assert t == 0x02
        vals.append(int.from_bytes(v, "big"))
    _, n, ee, d, p, q = vals[:6]
    assert ee == e and p * q == n and n.bit_length() == bits
    return {"bits": bits, "n": hex(n)[2:], "e": hex(e)[2:], "d": hex(d)[2:], "p": hex(p)[2:], "q": hex(q)[2:],
            "pkcs1_der": pub.hex()}


def main():
    keys = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            keys = json.load(f)
    plan = [("rsa2048", 2048, 16, 65537), ("rsa4096", 4096, 16, 65537), ("rsa1024", 1024, 2, 65537),
            ("rsa2048e3", 2048, 1, 3), ("rsa3072", 3072, 1, 65537),
            # moduli that do not fill their top byte / 32-bit limb / container (tests/rsa_edge_cases.py)
            ("rsa1025", 1025, 1, 65537), ("rsa2047", 2047, 1, 65537), ("rsa2049", 2049, 1, 65537),
            ("rsa3071", 3071, 1, 65537), ("rsa4095", 4095, 1, 65537), ("rsa2047e3", 2047, 1, 3)]
    for prefix, bits, cnt, e in plan:
        for i in range(cnt):
            name = f"{prefix}_{i:02d}"
            if name in keys:
                continue
            keys[name] = gen(bits, e)
            print(name, file=sys.stderr)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
