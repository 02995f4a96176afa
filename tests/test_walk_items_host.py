"""The small-scene walk's item derivation (kernels.hip, "Small scenes"), restated in numpy and checked on the host.

A block's work items are the set bits of its usable lanes' sweep masks, numbered lane by lane: lane l owns items
[excl[l], incl[l]) of the inclusive scan of the lanes' popcounts `rem`.  Node round k hands item g = 64 k + j to lane j, which
must find (owner, record) without any lane peeling its own bits:

  owner   a table of one entry per item of a window of 256 items is cleared; every lane with rem != 0 whose first item lies in
          the window writes (excl << 6) | lane at position excl - window base; an owner that began earlier and reaches into a
          round arrives as the `carry` -- the running maximum's value at lane 63 of the round before.  An inclusive running
          maximum over the round's 64 entries (entries grow with the lane, so one maximum yields both fields) gives every lane
          the entry of the interval it falls in: owner = entry & 63, rank r = g - (entry >> 6).  Lanes past the block's last
          item repeat that item and are inactive.
  record  from the block's top word down the set bits are counted; the word is the first at which the count exceeds r, the
          bit the (r - count above)-th set bit of that word from bit 0 up; bit 31 is the word's first record.  Slots below the
          block's first word may hold anything (the kernel reads 4 or 8 slots whatever the block's size): they are never chosen.

The derived items must be a permutation of the set bits, for any `rem`; three broken variants (a scan without the carry, a
rank off by one, `<=` for `<` in the word selection) must be caught by the same check.  This pins the specification the kernel's
comment cites; tests/test_gpu_walk_items.py drives the kernel itself."""
import numpy as np
import pytest

WINDOW, LANES = 256, 64


def derive_items(masks, slots=None, carry_on=True, rank_bias=0, word_le=False, garbage=None):
    """masks: (words, 64) uint32, zero rows for lanes that are not usable.  Returns the list of (owner, record) of the active
    lanes of every round, in round order, and the number of rounds."""
    words = masks.shape[0]
    slots = slots or (4 if words <= 4 else 8)
    rem = np.array([sum(bin(int(masks[w, l])).count("1") for w in range(words)) for l in range(LANES)], np.int64)
    incl = np.cumsum(rem)
    excl = incl - rem
    total = int(incl[-1])
    # the slots the kernel reads: the block's words at the top, whatever lies below its masks underneath
    rs = np.random.default_rng(5)
    below = rs.integers(0, 2 ** 32, (slots - words, LANES), dtype=np.uint64).astype(np.uint32) if garbage is None else np.full((slots - words, LANES), garbage, np.uint32)
    slot_words = np.concatenate([below, masks], 0)
    items, rounds, carry = [], 0, 0
    for base in range(0, total, WINDOW):
        table = np.zeros(WINDOW, np.int64)
        for l in range(LANES):
            if rem[l] != 0 and 0 <= excl[l] - base < WINDOW:
                table[excl[l] - base] = (int(excl[l]) << 6) | l
        for g0 in range(base, min(total, base + WINDOW), LANES):
            rounds += 1
            e = table[g0 - base:g0 - base + LANES].copy()
            if carry_on:
                e = np.maximum(e, carry)
            e = np.maximum.accumulate(e)
            carry = int(e[-1])
            take = min(total - g0, LANES)
            for j in range(LANES):
                act = j < take
                g = g0 + (j if act else take - 1)
                owner, r = int(e[j]) & 63, g - (int(e[j]) >> 6) + rank_bias
                cnt, above, sel, passed, found = 0, 0, 0, 0, False
                for i in range(slots - 1, -1, -1):
                    m = int(slot_words[i, owner])
                    if not found:
                        sel, above = m, cnt
                    cnt += bin(m).count("1")
                    found = (r <= cnt) if word_le else (r < cnt)
                    passed += 0 if found else 1
                r_in = r - above
                for _ in range(31):                       # the kernel's loop: at most 31 trips
                    if r_in > 0:
                        sel &= sel - 1
                        r_in -= 1
                bit = (sel & -sel).bit_length() - 1        # -1 for an empty word, as the instruction gives
                if act:
                    items.append((owner, (words - 1 - passed) * 32 + 31 - bit))
    return items, rounds


def set_bits(masks):
    return sorted((l, w * 32 + 31 - b) for w in range(masks.shape[0]) for l in range(LANES) for b in range(32) if (int(masks[w, l]) >> b) & 1)


def masks_for(rng, rem, words):
    """(words, 64) masks whose lane l holds rem[l] random bits"""
    m = np.zeros((words, LANES), np.uint32)
    for l, n in enumerate(rem):
        for p in rng.choice(words * 32, int(n), replace=False):
            m[p // 32, l] |= np.uint32(1 << (p % 32))
    return m


def _cases():
    rng = np.random.default_rng(1)
    out = {"all-zero": masks_for(rng, np.zeros(64, int), 4),
           "one-lane-256": masks_for(rng, np.eye(1, 64, 20, dtype=int)[0] * 256, 8),
           "all-lanes-1": masks_for(rng, np.ones(64, int), 4),
           "all-lanes-full": np.full((8, 64), 0xFFFFFFFF, np.uint32),
           "one-word-full": masks_for(rng, np.zeros(64, int), 4),
           "straddle-64": masks_for(rng, np.array([1] * 63 + [2]), 4),
           "two-owners-500": masks_for(rng, np.eye(1, 64, 20, dtype=int)[0] * 250 + np.eye(1, 64, 45, dtype=int)[0] * 250, 8)}
    out["one-word-full"][2, 7] = 0xFFFFFFFF
    for k, words in enumerate((1, 2, 3, 4, 5, 7, 8)):
        out[f"random-{words}w-sparse"] = masks_for(rng, rng.poisson(1.8, 64).clip(0, words * 32), words)
        out[f"random-{words}w-dense"] = masks_for(rng, rng.integers(0, words * 32 + 1, 64) * (rng.random(64) < 0.6), words)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_derived_items_are_a_permutation_of_the_set_bits(name):
    masks = CASES[name]
    want = set_bits(masks)
    for garbage in (None, 0, 0xFFFFFFFF):
        items, rounds = derive_items(masks, garbage=garbage)
        assert rounds == (len(want) + 63) // 64
        assert sorted(items) == want, name
    if masks.shape[0] <= 4:                                # a block of at most 4 words through the 8-slot form as well
        assert sorted(derive_items(masks, slots=8)[0]) == want


@pytest.mark.parametrize("broken", [dict(carry_on=False), dict(rank_bias=1), dict(rank_bias=-1), dict(word_le=True)],
                         ids=["scan-drops-the-carry", "rank-plus-one", "rank-minus-one", "word-selection-le"])
def test_broken_variants_are_rejected(broken):
    caught = [name for name, masks in CASES.items() if sorted(derive_items(masks, **broken)[0]) != set_bits(masks)]
    # every variant fails wherever an owner holds two items or more; the carry only where an owner spans two rounds
    assert caught, broken
    need = {"one-lane-256", "straddle-64", "two-owners-500"} if "carry_on" in broken else {"all-lanes-full", "one-lane-256", "random-4w-dense"}
    assert need <= set(caught), (broken, caught)
