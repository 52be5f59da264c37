"""extract_email_body against the reference's own outputs — once they exist.

`tests/golden/body_manifest.json` lists e-mails that sit on the behaviours of mailparse's get_body_raw this repository restated from
recollection (include/zkemail_amd.h, rules 5, 6, 8, 9).  `bindings/zkemail-core-amd/examples/dump_fixtures.rs`, run by anyone with
the zkemail.rs workspace and cargo, writes `extract_email_body`'s bytes (or its panic) for them into `tests/golden/ref/body/`.  With
that directory present the model (CPU tier) and the engine (`-m gpu`) are compared with it; without it these tests SKIP with
"parity unpinned", which is the state of this tree.  Always checked: the manifest is in step with its generator and the model has an
answer for every case."""
import json
import os
import subprocess
import sys

import pytest

import body_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(G, "body_manifest.json")))
REF = os.path.join(G, "ref", "body")
HAVE_REF = os.path.isdir(REF) and any(f.endswith(".json") for f in os.listdir(REF))
unpinned = pytest.mark.skipif(not HAVE_REF, reason="parity unpinned: tests/golden/ref/body/ is absent — run bindings/zkemail-core-amd/examples/"
                                                  "dump_fixtures.rs with a Rust toolchain to produce the reference's own outputs")


def raws():
    return [open(os.path.join(G, c["eml"]), "rb").read() for c in MANIFEST["cases"]]


def test_manifest_is_in_step_and_the_model_answers_every_case():
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "tools", "gen_body_manifest.py"), "--check"])
    assert r.returncode == 0, "tests/golden/body_manifest.json is stale: run python tools/gen_body_manifest.py"
    cases = MANIFEST["cases"]
    assert len(cases) >= 15 and len({c["name"] for c in cases}) == len(cases)
    kinds = [M.verdict(raw)[0] for raw in raws()]
    assert "undecided" not in kinds and "fail" not in kinds       # every case is one the reference decides and the engine answers
    assert kinds.count("decode") >= 3 and kinds.count("ok") >= 10
    for topic in ("EOL chop", "untrimmed CTE", "base64 without padding", "QP final line break", "unterminated last part"):
        assert any(topic in c["why"] for c in cases), topic


def _compare(answers, who):
    """answers[i]: ("ok", bytes) | ("panic",) for the manifest's e-mails, in order."""
    failures = []
    for c, a in zip(MANIFEST["cases"], answers):
        ref = json.load(open(os.path.join(REF, c["name"] + ".json")))
        want = ("ok", bytes.fromhex(ref["body_hex"])) if "body_hex" in ref else ("panic",)
        if a != want:
            failures.append((c["name"], c["why"], a, want))
    assert not failures, (who, failures)


@unpinned
def test_model_against_the_reference():
    out = []
    for raw in raws():
        v = M.verdict(raw)
        out.append(("ok", v[1].data) if v[0] == "ok" else ("panic",))
    _compare(out, "tests/body_model.py")


@unpinned
@pytest.mark.gpu
def test_engine_against_the_reference(engine):
    _compare([("ok", f.body) if f.status == 0 else ("panic",) for f in engine.extract_bodies(raws())], "zke_extract_bodies")
