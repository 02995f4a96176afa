"""The small-scene walk's hybrid numbering (kernels.hip, "Small scenes": round 0 in the lane, the cooperative rounds for the
rest), restated in numpy beside the model of the cooperative derivation in tests/test_walk_items_host.py and checked on the host.

  round 0   every usable lane with rem != 0 takes what the cooperative numbering calls its item 0: the top-most non-zero word of
            its block, and that word's lowest set bit (bit 31 is the word's first record).  Its own masks, its own ray: no table.
  the rest  the cooperative derivation on the reduced counts rem - 1: scan, table entries, windows, carry and the number of
            rounds all come from them; a lane that falls to an owner with rank r among the owner's REMAINING items picks item
            r + 1 of the owner's words, which still hold the bit round 0 took.  A reduced total of 0 runs no round at all.

Lanes that are not usable own nothing whatever their mask words hold (the kernel zeroes their count, not their words).  Round 0
plus the cooperative rounds must yield every set bit of the usable lanes exactly once; a variant that forgets the + 1 and one
that takes the first bit of the wrong word (the lowest non-zero one) must be caught by the same check.
tests/test_gpu_walk_first_item.py drives the kernel itself."""
import numpy as np
import pytest

from test_walk_items_host import LANES, WINDOW, derive_items, masks_for, set_bits


def _popcount(x):
    return bin(int(x)).count("1")


def derive_hybrid(masks, usable=None, skip=1, first_word="top", slots=None):
    """masks: (words, 64) uint32, usable: 64 booleans (default: all).  Returns the (owner, record) pairs of round 0, those of the
    cooperative rounds' active lanes in round order, and the number of cooperative rounds."""
    words = masks.shape[0]
    slots = slots or (4 if words <= 4 else 8)
    usable = np.ones(LANES, bool) if usable is None else np.asarray(usable, bool)
    rem = np.array([sum(_popcount(masks[w, l]) for w in range(words)) if usable[l] else 0 for l in range(LANES)], np.int64)
    round0 = []
    for l in range(LANES):
        if rem[l] != 0:
            nz = [w for w in range(words) if masks[w, l] != 0]
            w0 = max(nz) if first_word == "top" else min(nz)
            m = int(masks[w0, l])
            round0.append((l, w0 * 32 + 31 - ((m & -m).bit_length() - 1)))
    rest = rem - (rem != 0)
    incl = np.cumsum(rest)
    excl = incl - rest
    total = int(incl[-1])
    # the slots the kernel reads: the block's words at the top, whatever lies below its masks underneath
    below = np.random.default_rng(5).integers(0, 2 ** 32, (slots - words, LANES), dtype=np.uint64).astype(np.uint32)
    slot_words = np.concatenate([below, masks], 0)
    items, rounds, carry = [], 0, 0
    for base in range(0, total, WINDOW):
        table = np.zeros(WINDOW, np.int64)
        for l in range(LANES):
            if rest[l] != 0 and 0 <= excl[l] - base < WINDOW:
                table[excl[l] - base] = (int(excl[l]) << 6) | l
        for g0 in range(base, min(total, base + WINDOW), LANES):
            rounds += 1
            e = np.maximum.accumulate(np.maximum(table[g0 - base:g0 - base + LANES], carry))
            carry = int(e[-1])
            take = min(total - g0, LANES)
            for j in range(take):
                owner, r = int(e[j]) & 63, g0 + j - (int(e[j]) >> 6) + skip
                cnt, above, sel, passed, found = 0, 0, 0, 0, False
                for i in range(slots - 1, -1, -1):
                    m = int(slot_words[i, owner])
                    if not found:
                        sel, above = m, cnt
                    cnt += _popcount(m)
                    found = r < cnt
                    passed += 0 if found else 1
                for _ in range(min(r - above, 31)):
                    sel &= sel - 1
                items.append((owner, (words - 1 - passed) * 32 + 31 - ((sel & -sel).bit_length() - 1)))
    return round0, items, rounds


def _cases():
    rng = np.random.default_rng(2)
    out = {}
    for words in range(1, 9):
        for kind in ("sparse", "dense"):
            rem = rng.poisson(1.8, 64).clip(0, words * 32) if kind == "sparse" else rng.integers(0, words * 32 + 1, 64) * (rng.random(64) < 0.6)
            out[f"{words}w-{kind}"] = (masks_for(rng, rem, words), rng.random(64) < 0.7)
    out["one-each"] = (masks_for(rng, np.ones(64, int), 4), np.ones(64, bool))
    out["two-each"] = (masks_for(rng, np.full(64, 2), 2), np.ones(64, bool))
    out["reduced-65"] = (masks_for(rng, np.array([2] * 63 + [3]), 4), np.ones(64, bool))
    out["reduced-257"] = (masks_for(rng, np.array([5] * 63 + [6]), 8), np.ones(64, bool))
    out["one-lane-everything"] = (masks_for(rng, np.array([1] * 20 + [256] + [0] * 43), 8), np.ones(64, bool))
    out["all-full-every-other-lane-usable"] = (np.full((8, 64), 0xFFFFFFFF, np.uint32), np.arange(64) % 2 == 0)
    last = np.zeros((8, 64), np.uint32)
    last[7, 33] = 1                                          # the last record of the last word, nothing else
    out["last-record-only"] = (last, np.ones(64, bool))
    return out


CASES = _cases()


def _want(masks, usable):
    return set_bits(np.where(usable[None, :], masks, 0).astype(np.uint32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_round_0_and_the_cooperative_rounds_yield_every_set_bit_once(name):
    masks, usable = CASES[name]
    want = _want(masks, usable)
    round0, items, rounds = derive_hybrid(masks, usable)
    owners = sorted({l for l, _ in want})
    assert sorted(l for l, _ in round0) == owners                          # one item per owner, and only owners
    assert rounds == (len(want) - len(owners) + 63) // 64                 # none when no lane holds a second candidate
    assert sorted(round0 + items) == want, name
    if masks.shape[0] <= 4:                                                # a block of at most 4 words through the 8-slot form as well
        r0, it, _ = derive_hybrid(masks, usable, slots=8)
        assert sorted(r0 + it) == want


@pytest.mark.parametrize("name", sorted(k for k, (m, u) in CASES.items() if u.all()))
def test_the_hybrid_takes_the_items_of_the_cooperative_model(name):
    """round 0 takes the cooperative numbering's item 0 of every owner; the union is the imported model's"""
    masks, _ = CASES[name]
    coop, _ = derive_items(masks)
    round0, items, _ = derive_hybrid(masks)
    assert sorted(round0 + items) == sorted(coop)
    first = {}
    for owner, rec in coop:                                                # lane by lane, every owner's items in rank order
        first.setdefault(owner, rec)
    assert dict(round0) == first


def test_named_shapes():
    assert derive_hybrid(*CASES["one-each"])[2] == 0
    assert derive_hybrid(*CASES["two-each"])[2] == 1
    assert derive_hybrid(*CASES["reduced-65"])[2] == 2
    assert derive_hybrid(*CASES["reduced-257"])[2] == 5
    r0, items, rounds = derive_hybrid(*CASES["last-record-only"])
    assert (r0, items, rounds) == ([(33, 255)], [], 0)


@pytest.mark.parametrize("broken", [dict(skip=0), dict(first_word="bottom")], ids=["forgets-the-plus-one", "first-bit-of-the-wrong-word"])
def test_broken_variants_are_rejected(broken):
    caught = [name for name, (masks, usable) in CASES.items()
              if sorted(sum(derive_hybrid(masks, usable, **broken)[:2], [])) != _want(masks, usable)]
    assert caught, broken
    # without the + 1 every owner of two items repeats its first and drops its last; the wrong word shows wherever an owner's
    # candidates lie in two words
    need = {"two-each", "reduced-65", "all-full-every-other-lane-usable"} if "skip" in broken else {"8w-dense", "all-full-every-other-lane-usable", "one-lane-everything"}
    assert need <= set(caught), (broken, caught)
    # and neither is caught where no lane has a second candidate: round 0 alone is right in both
    if "skip" in broken:
        assert "one-each" not in caught and "last-record-only" not in caught
