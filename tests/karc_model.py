"""An independent model of the dropping of arcs to weak k-mers (include/soapdenovo2_amd.h, pg_kindex_drop_weak_arcs), written from the rule
and sharing no code with the library: the index is kindex_model.Model's dict from canonical k-mer (a Python int) to cnt word, which a
round changes in place; an oriented k-mer is ktip_model's pair (its value, its reverse complement's value) of Python ints.

  * the arc of a solid oriented k-mer r by base b exists when r's out-counter for b is >= min_arc; it is dangling when r[1:] + [b] is not
    solid: the dict has no such key, its word is 0, or its coverage is below min_cov
  * a round finds every dangling arc on the dict as it stood, then sets each one's out-counter to 0 in r's own word: right counter b of the
    word when r is its canonical form, else left counter b ^ 2.  Nothing else changes
  * a side is the pair (canonical key, orientation); it is a candidate when ktip_model.side gives BRANCH_OUT or WEAK_NEXT for it, pruned
    when it holds a dangling arc and kept otherwise

drop_round() asserts for itself that every side with a dangling arc is such a candidate, that no word but a pruned side's changes and that
no k-mer changes between solid and not."""
import ktip_model as T


def dangling(cnt, K, r, min_cov, min_arc):
    """The bases whose arc out of the solid oriented k-mer r dangles."""
    outs = T.out_counters(cnt[T.key_of(r)], T.is_fwd(r))
    return [b for b in range(4) if outs[b] >= min_arc and not T.solid(cnt.get(T.key_of(T.step(r, b, K)), 0), min_cov)]


def sides(cnt, K, min_cov, min_arc):
    """Every candidate side of the dict as (r, its dangling bases)."""
    out = []
    for key in sorted(k for k, w in cnt.items() if T.solid(w, min_cov)):
        x = T.node_of_key(key, K)
        for r in (x, T.flip(x)):
            bases = dangling(cnt, K, r, min_cov, min_arc)
            if T.side(cnt, K, r, min_cov, min_arc)[0] in (T.BRANCH_OUT, T.WEAK_NEXT):
                out.append((r, bases))
            else:
                assert not bases, "a dangling arc on a side that is neither BRANCH_OUT nor WEAK_NEXT"
    return out


def drop_round(model, min_cov, min_arc):
    """One round on model.cnt, in place: (totals [sides pruned, arcs cleared, solid before, sides kept], the set of removed keys -- always
    empty --, the list of (key, which half -- 0 low --, which counter of it) cleared)."""
    K, cnt = model.K, model.cnt
    before = dict(cnt)
    n_solid = sum(1 for w in before.values() if T.solid(w, min_cov))
    pruned, kept, cleared = 0, 0, []
    for r, bases in sides(before, K, min_cov, min_arc):
        if not bases:
            kept += 1
            continue
        pruned += 1
        for b in bases:
            half, idx = (1, b) if T.is_fwd(r) else (0, b ^ 2)
            cnt[T.key_of(r)] &= ~(63 << (32 * half + 6 * idx))
            cleared.append((T.key_of(r), half, idx))
    touched = {k for k, _, _ in cleared}
    for k, w in before.items():
        assert k in touched or cnt[k] == w, "a word that is no pruned side's changed"
        assert T.solid(cnt[k], min_cov) == T.solid(w, min_cov), "a k-mer changed between solid and weak"
    return [pruned, len(cleared), n_solid, kept], set(), cleared
