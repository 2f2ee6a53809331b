"""An independent model of the dropping of short isolated unitigs (include/soapdenovo2_amd.h, pg_kindex_drop_isolated), written from the
rule and sharing no code with the library: the index is kindex_model.Model's dict from canonical k-mer (a Python int) to cnt word, which
a round changes in place; oriented k-mers, the counters, solid and the side test are ktip_model's, arithmetic on Python ints.

  * free: a side whose reason is DEAD_END or WEAK_NEXT
  * an island: from an oriented solid k-mer whose left side is free, to the right through open sides, at most max_len k-mers, to a
    right side that is free.  Every other ending -- BRANCH_IN (a tip), BRANCH_OUT, HAIRPIN, more than max_len k-mers -- is none, and a
    ring has no k-mer with an end side
  * removed: the sum of the members' coverage bytes (bits 31:24 of the word) is at most max_cov a member
  * a round finds every island on the dict as it stood, then every k-mer of a removed island gets the word 0; nothing else changes

The library decides an island from one of its two ends by an order on the end k-mers.  The model has no such rule: it walks from every
free side, so it meets an island twice, once from either end (the same member keys, reversed), and counts the set of members once.
isolated_round() asserts that every island was met exactly twice, that no k-mer lies twice in one island and that each removed key lay
in exactly one removed island."""
import ktip_model as T

FREE = (T.DEAD_END, T.WEAK_NEXT)


def coverage(w):
    return (w >> 24) & 0xFF


def islands(cnt, K, min_cov, min_arc, max_len):
    """Every island of the dict, once: a list of member-key lists (from one end to the other), in the order of their least key."""
    met = {}
    for key in sorted(k for k, w in cnt.items() if T.solid(w, min_cov)):
        for x0 in (T.node_of_key(key, K), T.flip(T.node_of_key(key, K))):
            if T.side(cnt, K, T.flip(x0), min_cov, min_arc)[0] not in FREE:
                continue
            x, members = x0, [key]
            while True:
                reason, y = T.side(cnt, K, x, min_cov, min_arc)
                if not reason and len(members) == max_len:
                    reason = T.TOO_LONG
                if reason:
                    break
                members.append(T.key_of(y))
                x = y
            if reason in FREE:
                assert len(set(members)) == len(members), "a k-mer lies twice in one island"
                met.setdefault(frozenset(members), []).append(members)
    for walks in met.values():
        assert len(walks) == 2 and walks[0] == walks[1][::-1], "an island is met once from either end"
    return sorted((walks[0] for walks in met.values()), key=min)


def isolated_round(model, min_cov, min_arc, max_len, max_cov):
    """One round on model.cnt, in place: (totals [islands removed, k-mers removed, solid before, islands kept], the set of removed
    keys)."""
    K, cnt = model.K, model.cnt
    before = dict(cnt)
    n_solid = sum(1 for w in before.values() if T.solid(w, min_cov))
    gone, kept = [], 0
    for members in islands(before, K, min_cov, min_arc, max_len):
        if sum(coverage(before[k]) for k in members) <= max_cov * len(members):
            gone.append(members)
        else:
            kept += 1
    removed = set()
    for members in gone:
        assert not removed & set(members), "a removed key lies in two removed islands"
        removed.update(members)
    assert len(removed) == sum(len(m) for m in gone)
    for k in removed:
        cnt[k] = 0
    return [len(gone), len(removed), n_solid, kept], removed
