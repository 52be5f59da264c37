"""CPU (-m "not gpu"): the hash stage's job mapping restated step for step — sha_len_class and sha_pick_job (csrc/sha256.hip.h),
sha_bucket (csrc/parse.hip.h), the tile hand-over of fetch / commit — and the census of what the populations of
tests/sha_edge_cases.py make the three SHA routines do.  tests/test_gpu_sha_edges.py runs exactly these populations, so a
GPU test cannot pass while a branch listed here is left out.  Every comparison is for equality.

Routines and what selects them:
  batch   sha256_batch_kernel: one wave per 64 messages in arrival order (launches above 512 groups, or sha_mapping = 1)
  pair2   sha256_pair_group, two waves (feeder + rounds): groups without a SHA-1 job
  pair1   sha256_pair_group, its one-wave fallback: groups with at least one SHA-1 job
  lane    sha_lane: one lane per message, later signature rounds
In a batch the pair routine maps lanes to jobs per kind (0 body, 1 header preimage): directly when the populated length
classes span at most two neighbours, else through the length buckets."""
import random
from collections import defaultdict

import numpy as np
import pytest

import sha_edge_cases as S

SHA_CLASSES = 192
KEY_NONE = 0xFFFFFFFF
T = S.SHA_TILE
DIRECT = "direct"


def sha_len_class(nblk):
    if nblk < 16:
        return nblk
    e = nblk.bit_length() - 1                                  # 31 - clz
    return 16 + (e - 4) * 8 + ((nblk >> (e - 3)) & 7)


def sha_bucket(lengths, arrival=None):
    """the front end's filing of one kind: lengths[i] is None for an e-mail without a message -> (cnt[192], key[n]).
    `arrival`: the order in which the atomic adds land (any order is possible on the device)"""
    cnt = [0] * SHA_CLASSES
    key = [KEY_NONE] * len(lengths)
    for i in (arrival if arrival is not None else range(len(lengths))):
        if lengths[i] is None:
            continue
        c = sha_len_class(S.nblk(lengths[i]))
        key[i] = (c << 24) | (cnt[c] & 0xFFFFFF)
        cnt[c] += 1
    return cnt, key


def sha_pick_job(cnt, key, g, stats=None):
    """One group's 64 picks, as the feeder wave works them out: -> DIRECT, None (skip) or [job or KEY_NONE] * 64"""
    n = len(key)
    c3 = [[cnt[3 * lane + k] for k in range(3)] for lane in range(64)]
    tot3 = [sum(x) for x in c3]
    nonempty = [lane for lane in range(64) if tot3[lane]]
    if not nonempty:
        return None
    lo_lane, hi_lane = nonempty[0], nonempty[-1]
    lo = min(3 * lo_lane + k for k in range(3) if c3[lo_lane][k])
    hi = max(3 * hi_lane + k for k in range(3) if c3[hi_lane][k])
    if stats is not None:
        stats["spread"] = hi - lo
        stats["cross_triple"] = lo_lane != hi_lane
    if hi - lo <= 1:
        return DIRECT
    above = list(tot3)                                         # inclusive suffix sum over the lanes, by doubling shifts
    o = 1
    while o < 64:
        above = [above[l] + (above[l + o] if l + o < 64 else 0) for l in range(64)]
        o <<= 1
    total = above[0]
    if 64 * g >= total:
        return None
    pick = [0] * (SHA_CLASSES + 64)
    for lane in range(64):
        b = above[lane] - tot3[lane]
        pick[3 * lane + 2] = b; b += c3[lane][2]
        pick[3 * lane + 1] = b; b += c3[lane][1]
        pick[3 * lane + 0] = b
        pick[SHA_CLASSES + lane] = KEY_NONE
    base = 64 * g
    for t0 in range(0, n, 256):
        for q in range(4):
            for lane in range(64):
                i = t0 + 64 * q + lane
                k = key[i] if i < n else KEY_NONE
                if k != KEY_NONE:
                    gp = (pick[k >> 24] + (k & 0xFFFFFF) - base) & 0xFFFFFFFF
                    if gp < 64:
                        assert pick[SHA_CLASSES + gp] == KEY_NONE, "two messages at one position"
                        pick[SHA_CLASSES + gp] = i
    return pick[SHA_CLASSES:]


def kind_groups(lengths, arrival=None, stats=None):
    """The groups of one kind of a batch under the pair routine: [(g, [job index or None] * 64)], skipped groups left out"""
    n = len(lengths)
    n_pad = (n + 63) & ~63
    cnt, key = sha_bucket(lengths, arrival)
    out = []
    for g in range(n_pad // 64):
        st = {}
        p = sha_pick_job(cnt, key, g, st)
        if stats is not None:
            stats.setdefault("mapping", DIRECT if p == DIRECT else "bucketed")
            stats.update(st)
            stats.setdefault("skipped", 0)
            stats["skipped"] += p is None
        if p is None:
            continue
        if p == DIRECT:
            p = [64 * g + l if 64 * g + l < n and lengths[64 * g + l] is not None else None for l in range(64)]
        else:
            p = [None if j == KEY_NONE else j for j in p]
        out.append((g, p))
    return out


# ------------------------------------------------------------------ properties of the mapping
def adversarial_populations():
    rng = random.Random(2026)
    pops = []
    for n in (1, 63, 64, 65, 255, 256, 257, 700, 1000, 1029):
        pops.append([rng.choice([0, 55, 56, 119, 120, 500, 5000, 70000, 10 ** 6]) for _ in range(n)])
        pops.append([None if rng.random() < 0.4 else int(2 ** rng.uniform(0, 21)) for _ in range(n)])
        pops.append([None if rng.random() < 0.9 else rng.choice([100, 300, 900]) for _ in range(n)])       # fewer messages than groups
    pops.append([None] * 130)
    pops.append([120] * 100 + [184] * 100)                      # classes 3 and 4: direct
    pops.append([56] * 100 + [184] * 100)                       # classes 2 and 4: bucketed
    pops.append([64 * c - 9 for c in range(1, 40)] * 5)         # one message more per class than lanes in some groups
    return pops


@pytest.mark.parametrize("ix", range(len(adversarial_populations())))
def test_every_message_is_picked_exactly_once(ix):
    lengths = adversarial_populations()[ix]
    n = len(lengths)
    for arrival in (None, random.Random(ix).sample(range(n), n)):
        cnt, key = sha_bucket(lengths, arrival)
        total = sum(cnt)
        assert total == sum(x is not None for x in lengths)
        seen = []
        direct = False
        for g in range(((n + 63) & ~63) // 64):
            p = sha_pick_job(cnt, key, g)
            if p == DIRECT:
                direct = True
                continue
            assert not direct                                   # the decision is the batch's, not the group's
            if total == 0 or 64 * g >= total:
                assert p is None, g
                continue
            assert p is not None
            got = [j for j in p if j != KEY_NONE]
            assert len(got) == min(64, total - 64 * g)          # full groups, then one cut by the total
            assert all(key[j] != KEY_NONE for j in got)         # an e-mail without a message is never picked
            cls = [key[j] >> 24 for j in got]
            assert cls == sorted(cls, reverse=True)             # longest class first, lane by lane
            seen += got
        if not direct:
            assert sorted(seen) == [i for i in range(n) if lengths[i] is not None]


def test_len_class_range_and_monotony():
    assert [sha_len_class(b) for b in range(16)] == list(range(16))
    prev = 0
    probes = list(range(1, 5000)) + [2 ** k + d for k in range(4, 26) for d in (-1, 0, 1)] + [(2 ** 31 - 1 + 72) >> 6]
    for b in sorted(probes):
        c = sha_len_class(b)
        assert prev <= c and (c <= prev + 1 or b > 5000)        # monotone; no class jumped over where the probes are dense
        prev = c
    # the front end refuses e-mails of 2^31 bytes and more: the largest class in use is 184, and class 191 — whose counter
    # slot the pair routine borrows for its skip flag — is never a counter in use
    assert sha_len_class(S.nblk(2 ** 31 - 1)) == 184 < SHA_CLASSES - 1
    for b in (16, 17, 31, 32, 1000, 2 ** 25):                  # a class holds block counts within 12.5 % of each other
        same = [x for x in range(b, b + b // 8 + 2) if sha_len_class(x) == sha_len_class(b)]
        assert max(same) <= b * 1.125


# ------------------------------------------------------------------ the census
def message_features(length):
    f = {f"mod64={length % 64}"} if length % 64 in (55, 56, 63, 0) else set()
    if length % 16:
        f.add(f"rem={length % 16}")                             # the last chunk takes the byte loads
    last = S.nblk(length) - 1
    if length // T != (last * 64 + 56) // T:
        f.add("split")                                          # 0x80 in tile t, the bit length in tile t + 1
    return f


def group_features(rows):
    """rows: the (length, sha1) or None of a wave's 64 lanes"""
    f = set()
    nb = [S.nblk(r[0]) if r else 0 for r in rows]
    for blk0 in range(0, max(nb), T // 64):
        live = [blk0 < x for x in nb]
        if any(live[r] != live[r + 1] for r in range(63)):
            f.add("finished_next_to_live")
    if len({r[1] for r in rows if r}) == 2:
        f.add("mixed_algorithms")
    if any(r is None for r in rows):
        f.add("inactive_rows")
    return f


def census(groups, routine_of):
    """{(routine, algo): features} over waves of 64 rows; routine_of(rows) names the routine a wave takes"""
    out = defaultdict(set)
    for rows in groups:
        rt = routine_of(rows)
        gf = group_features(rows)
        for r in rows:
            if r:
                out[(rt, "sha1" if r[1] else "sha256")] |= message_features(r[0]) | gf
    return out


def arrival_groups(rows):
    return [rows[i:i + 64] + [None] * (64 - len(rows[i:i + 64])) for i in range(0, len(rows), 64)]


def pair_routine(rows):
    return "pair1" if any(r and r[1] for r in rows) else "pair2"


ALL_REMS = {f"rem={k}" for k in range(1, 16)}
PAD_EDGES = {"mod64=55", "mod64=56", "mod64=63", "mod64=0"}
TILE_FEATURES = PAD_EDGES | ALL_REMS | {"split", "finished_next_to_live"}


def batch_job_rows(pop, kinds=(0, 1)):
    """the kind-major job list of a batch, kinds 0 and 1 (what sha256_batch_kernel sees in arrival order)"""
    n_pad = (len(pop) + 63) & ~63
    rows = []
    for k in kinds:
        rows += [None if p is None else (p[k], p[2]) for p in pop] + [None] * (n_pad - len(pop))
    return rows


def pair_rows(pop, stats):
    """the waves of a batch under the pair routine, kinds 0 and 1; stats[kind] = the mapping's own census"""
    out = []
    for k in (0, 1):
        lengths = [None if p is None else p[k] for p in pop]
        for g, picks in kind_groups(lengths, None, stats.setdefault(k, {})):
            rows = [None if j is None else (pop[j][k], pop[j][2]) for j in picks]
            stats[k].setdefault("spans", []).append(len({sha_len_class(S.nblk(r[0])) for r in rows if r}))
            stats[k].setdefault("fills", []).append(sum(r is not None for r in rows))
            stats[k].setdefault("classes", set()).update(sha_len_class(S.nblk(r[0])) for r in rows if r)
            out.append(rows)
    return out


@pytest.fixture(scope="module")
def block_set():
    msgs, info = S.block_message_set(S.N_BLOCK)
    return [(len(m), False) for m in msgs], info


def test_census_block_level(block_set):
    """GPU tests 1 and 2: zke_sha256_batch over S.block_message_set — SHA-256 only, direct mapping."""
    rows, info = block_set
    n = len(rows)
    assert n > 32768 and 64 < n % 256 <= 128                    # the one-wave kernel; its last workgroup: a full wave, a partly
    assert S.N_BLOCK_CUT < 32768 and 64 < S.N_BLOCK_CUT % 256 <= 128 and S.N_BLOCK_CUT >= info["n_edge"]   # filled one, two empty
    for cut, routine in ((n, "batch"), (n, "pair2"), (S.N_BLOCK_CUT, "batch")):
        c = census(arrival_groups(rows[:cut]), lambda r: routine)
        assert c[(routine, "sha256")] >= TILE_FEATURES | {"inactive_rows"}, (routine, TILE_FEATURES - c[(routine, "sha256")])
    # every edge length at every start alignment
    msgs, starts = S.aligned_messages()
    at = defaultdict(set)
    for m, s in zip(msgs[1::2], starts[1::2]):
        at[len(m)].add(s % 16)
    assert all(at[L] == set(range(16)) for L in S.EDGE_LENS)
    for name, first in info["pops"]:
        assert first % 64 == 0
    thr, _ = S.block_message_set(32769, max_len=70000)
    c = census(arrival_groups([(len(m), False) for m in thr[:32768]]), lambda r: "pair2")
    assert c[("pair2", "sha256")] >= TILE_FEATURES


@pytest.fixture(scope="module")
def pipe_pop():
    emails, inter = S.pipeline_population()
    for a in ("rsa-sha256", "rsa-sha1"):      # from_domain (kind 2, always SHA-256) at its padding edges, beside bodies of either algorithm
        assert {len(e.from_domain) for e, it in zip(emails, inter) if it["algo"] == a} >= {55, 56, 63, 64}
    return S.population_lengths(inter)


def test_census_pipeline_population(pipe_pop):
    """GPU test 3: one batch, both algorithms in every group of 64 e-mails."""
    pop = pipe_pop
    for g in range(0, len(pop), 64):
        assert len({p[2] for p in pop[g:g + 64]}) == 2
    hl = sorted({p[1] for p in pop if p[2]} & {p[1] for p in pop if not p[2]})
    assert max(b - a for a, b in zip(hl, hl[1:])) == 1 and len(hl) >= 130          # consecutive preimage lengths, both algorithms
    # sha_mapping = 1: the one-wave kernel over the job list in arrival order
    c = census(arrival_groups(batch_job_rows(pop)), lambda r: "batch")
    for algo in ("sha256", "sha1"):
        assert c[("batch", algo)] >= TILE_FEATURES | {"mixed_algorithms"}, (algo, TILE_FEATURES - c[("batch", algo)])
    # default engine: the pair routine; a group with a SHA-1 job takes its one-wave fallback
    stats = {}
    c = census(pair_rows(pop, stats), pair_routine)
    assert stats[0]["mapping"] == "bucketed" and stats[1]["mapping"] == "bucketed"
    for algo in ("sha256", "sha1"):
        assert c[("pair1", algo)] >= TILE_FEATURES | {"mixed_algorithms"}, (algo, TILE_FEATURES - c[("pair1", algo)])


def test_census_header_sweep_keeps_the_direct_mapping():
    """GPU test 3, second batch: SHA-1 and SHA-256 padding edges of the header preimage under the direct mapping."""
    pop = S.population_lengths(S.header_sweep()[1])
    stats = {}
    c = census(pair_rows(pop, stats), pair_routine)
    assert stats[0]["mapping"] == DIRECT and stats[1]["mapping"] == DIRECT
    assert stats[0]["spread"] == 1 and stats[1]["spread"] == 1
    for algo in ("sha256", "sha1"):
        assert c[("pair1", algo)] >= PAD_EDGES | ALL_REMS | {"split", "mixed_algorithms"}


def test_census_bucket_populations():
    """GPU test 4: what the length-bucket populations reach, item by item."""
    pops = {k: S.population_lengths(v[1]) for k, v in S.bucket_populations().items()}
    st = {}
    for name, pop in pops.items():
        st[name] = {}
        pair_rows(pop, st[name])
    d = st["direct_two_classes"][0]                             # bodies: classes 2 and 3 — lane 0's triple and lane 1's
    assert d["mapping"] == DIRECT and d["spread"] == 1 and d["cross_triple"]
    b = st["bucketed_spread_two"][0]
    assert b["mapping"] == "bucketed" and b["spread"] == 2
    r = st["ragged_with_invalid"]
    assert len(pops["ragged_with_invalid"]) % 256 != 0 and any(p is None for p in pops["ragged_with_invalid"])
    for k in (0, 1):
        assert r[k]["mapping"] == "bucketed"
        assert 0 < r[k]["fills"][-1] < 64                       # a group cut by the number of messages
    assert max(r[0]["spans"]) >= 3                              # a group that holds three classes and more
    assert max(r[0]["classes"]) >= 16 and min(r[0]["classes"]) < 16
    s = st["skipped_groups"]
    assert s[0]["mapping"] == "bucketed" and s[0]["skipped"] >= 1 and len(pops["skipped_groups"]) % 256 != 0
    big = S.population_lengths(S.uniform_batch()[1])
    u = {}
    pair_rows(big, u)
    assert u[0]["mapping"] == DIRECT and u[0]["spread"] == 0    # the batch that follows: one class per kind


def test_census_signature_rounds():
    """GPU test 6: what sha_lane hashes — the good signature's body and header preimage, one lane each."""
    cs, nbad = S.signature_round_emails()
    assert set(nbad) == {1, 3}
    feats = defaultdict(set)
    hdr = defaultdict(set)
    for c, nb in zip(cs, nbad):
        a = "sha1" if c.inter["algo"] == "rsa-sha1" else "sha256"
        assert c.inter["hashed_body_len"] < len(c.inter["canon_body"])            # l= is shorter than the body
        for L in (c.inter["hashed_body_len"], len(c.inter["canon_header"])):
            feats[a] |= {f"mod64={L % 64}", f"mod4={L % 4}", f"nbad={nb}"}
        hdr[a].add(len(c.inter["canon_header"]))
        feats[a].add(f"body={c.inter['hashed_body_len']}")
    for a in ("sha256", "sha1"):
        assert feats[a] >= {f"mod64={k}" for k in range(64)} | {f"mod4={k}" for k in range(4)} | {"nbad=1", "nbad=3"}
        assert feats[a] >= {f"body={L}" for L in S.PIPE_BODY_LENS}
        h = sorted(hdr[a])
        run = best = 1
        for x, y in zip(h, h[1:]):
            run = run + 1 if y == x + 1 else 1
            best = max(best, run)
        assert best >= 130
