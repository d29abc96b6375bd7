"""CPU: a numpy restatement of the device's DropPath draw (csrc/common.h: philox4x32_7, drop_threshold, drop_path_factor) and of the
live table built from it (include/modaltune_hip.h: mt_droppath_live).  tests/test_droppath_skip_gpu.py compares the device table with
it and uses it, at collection time, to pick seeds whose draws cover the cases it needs."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32(ctr, key, rounds=7):
    """Philox4x32 (Salmon et al. 2011) with `rounds` rounds on python ints; the kernels use 7."""
    c0, c1, c2, c3 = (int(c) & MASK for c in ctr)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> 32, p0 & MASK, p1 >> 32, p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def rng_words(seed, step):
    """Engine.set_stochastic's device words {seed_lo, seed_hi, step, 0} after `step` mt_rng_advance launches."""
    return seed & 0x7FFFFFFF, (seed >> 31) & 0x7FFFFFFF, step & MASK, 0


def drop_threshold(p):
    v = np.float32(p) * np.float32(4294967296.0)           # fp32 product, as on the device
    return int(min(v, np.float32(4294967040.0)))


def path_live(rng, path_site, path_p, b):
    """drop_path_factor(...) != 0 for task pass b."""
    if not path_p > 0.0:
        return True
    r = philox4x32((b, W0, path_site, rng[2]), (rng[0], rng[1]))
    return r[0] >= drop_threshold(path_p)


def live_pattern(rng, path_site, path_p, B):
    return [path_live(rng, path_site, path_p, b) for b in range(B)]


def hull(pattern):
    live = [b for b, v in enumerate(pattern) if v]
    return (live[0], live[-1] + 1) if live else (0, 0)


def live_table(rng, sites, ps, B):
    return np.array([hull(live_pattern(rng, s, p, B)) for s, p in zip(sites, ps)], dtype=np.int32).reshape(len(sites), 2)


def layer_sites(depth, site_base=0):
    """Path sites of the backbone branches in table order (Engine._layer_drops): attention of layer 0, FFN of layer 0, ..."""
    return [s + 4 * l + site_base for l in range(depth) for s in (17, 19)]


def layer_ps(depth, drop_path_rate):
    dpr = np.linspace(0.0, float(drop_path_rate), depth) if depth > 1 else np.zeros(1)
    return [float(dpr[l]) for l in range(depth) for _ in range(2)]


def case_of(pattern):
    """none / first / last / middle / all dead (first and last may both hold for one pattern)."""
    B, dead = len(pattern), [not v for v in pattern]
    if not any(dead):
        return {"none"}
    if all(dead):
        return {"all"}
    out = set()
    if dead[0]:
        out.add("first")
    if dead[-1]:
        out.add("last")
    if B == 3 and dead == [False, True, False]:
        out.add("middle")
    return out


def possible_cases(B):
    return {"none", "all"} | ({"first", "last"} if B >= 2 else set()) | ({"middle"} if B == 3 else set())


def cases_seen(seed, step, depth, drop_path_rate, B, site_base=0):
    """{("attn" | "ffn", case)} over the layers with a DropPath rate > 0."""
    rng, seen = rng_words(seed, step), set()
    for i, (s, p) in enumerate(zip(layer_sites(depth, site_base), layer_ps(depth, drop_path_rate))):
        if p > 0.0:
            seen |= {("ffn" if i & 1 else "attn", c) for c in case_of(live_pattern(rng, s, p, B))}
    return seen


def pick_seeds(want, seen_of, limit, candidates=range(1, 4000)):
    """Greedy cover: the fewest seeds (at most `limit`) whose seen_of(seed) sets cover `want`."""
    left, picked = set(want), []
    pool = {s: seen_of(s) & left for s in candidates}
    while left:
        best = max(pool, key=lambda s: (len(pool[s] & left), -s))
        if not pool[best] & left:
            raise AssertionError(f"no seed covers {sorted(left)}")
        picked.append(best)
        left -= pool[best]
    assert len(picked) <= limit, (picked, limit)
    return picked


# ---------------------------------------------------------------------------------------------------------------- tests
def test_philox_known_answers():
    """Random123's known-answer vectors for Philox4x32-10: the round function, the key schedule and the word order."""
    assert philox4x32((0, 0, 0, 0), (0, 0), 10) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32((MASK,) * 4, (MASK, MASK), 10) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), 10) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    assert philox4x32((1, 2, 3, 4), (5, 6)) != philox4x32((1, 2, 3, 4), (5, 6), 10)


def test_threshold_and_rate():
    assert drop_threshold(0.0) == 0 and drop_threshold(0.5) == 1 << 31 and drop_threshold(1.0) == 4294967040
    rng = rng_words(77, 3)
    for p in (0.3, 0.6):
        dead = sum(not path_live(rng, 21, p, b) for b in range(4000))
        assert abs(dead / 4000 - p) < 0.03, (p, dead)
    assert all(path_live(rng, 17, 0.0, b) for b in range(8))


def test_hull_and_cases():
    assert hull([True, True, True]) == (0, 3) and hull([False, False]) == (0, 0) and hull([False, True, True]) == (1, 3)
    assert hull([True, False, False]) == (0, 1) and hull([True, False, True]) == (0, 3) and hull([False, True, False]) == (1, 2)
    assert case_of([True, False, True]) == {"middle"} and case_of([False, True, False]) == {"first", "last"}
    assert case_of([False]) == {"all"} and case_of([True, True]) == {"none"} and case_of([False, False, True]) == {"first"}
    t = live_table(rng_words(5, 1), layer_sites(3), layer_ps(3, 0.6), 3)
    assert t.shape == (6, 2) and (t[:2] == [0, 3]).all()          # layer 0: rate 0, every pass live
    assert ((0 <= t[:, 0]) & (t[:, 0] <= t[:, 1]) & (t[:, 1] <= 3)).all()


def test_seed_picker_covers_every_case_with_few_seeds():
    for B in (1, 2, 3):
        want = {(k, c) for k in ("attn", "ffn") for c in possible_cases(B)}
        seen_of = lambda s, B=B: cases_seen(s, 1, 3, 0.6, B)
        seeds = pick_seeds(want, seen_of, 4)
        assert set().union(*(seen_of(s) for s in seeds)) >= want
