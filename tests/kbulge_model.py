"""An independent model of bubble popping on strongest paths (include/soapdenovo2_amd.h, pg_kindex_pop_bulges), written from the rule and
sharing no code with the library: the index is kindex_model.Model's dict from canonical k-mer (a Python int) to cnt word, which a round
changes in place; an oriented k-mer is ktip_model's pair of Python ints, the side test is ktip_model.side, and an arm is
kbubble_model.branches' branch.  Where the library decides an arm from one of its starts, the model lists every arm of the graph first.

  * a strong step x -> y: b is the one base whose raw out-counter in x's word is >= min_arc and strictly greater than the other three;
    y = x[1:] + [b] is solid; canon(y) != canon(x); y's raw in-counter for x[0] is >= min_arc and strictly greater than y's other three
  * the strongest path S of an arm (u, v, members): strong steps from u; it succeeds at v (the same oriented k-mer), fails where there is
    no strong step, at canon(u) or canon(v) otherwise, or when it would hold more than len(members) + max_diff k-mers
  * minor: S succeeds, holds at least one k-mer, its first is not the arm's first, the lengths are within max_diff, and
    cov_P * len(S) < cov_S * len(P).  An arm is decided in the orientation whose first k-mer is not greater than the reverse complement of
    its last
  * a round decides every arm on the dict as it stood, then applies as kbubble_model.pop_round does

bulge_round() asserts for itself that no junction is a removed key, that no k-mer lies in two popped arms, that no k-mer of any S that
justified a pop is removed, and that after the round every such u still reaches its v by strong steps."""
import kbubble_model as B
import ktip_model as T


def strict_top(counters, min_arc):
    """The index of the counter that is >= min_arc and strictly greater than the others, or None."""
    top = max(counters)
    return counters.index(top) if top >= min_arc and counters.count(top) == 1 else None


def strong_step(cnt, K, x, min_cov, min_arc):
    """The k-mer behind the strong step out of the solid oriented k-mer x, or None."""
    b = strict_top(T.out_counters(cnt[T.key_of(x)], T.is_fwd(x)), min_arc)
    if b is None:
        return None
    y = T.step(x, b, K)
    wy = cnt.get(T.key_of(y), 0)
    if not T.solid(wy, min_cov) or T.key_of(y) == T.key_of(x):
        return None
    return y if strict_top(T.in_counters(wy, T.is_fwd(y)), min_arc) == T.first_base(x, K) else None


def strongest_path(cnt, K, u, v, most, min_cov, min_arc):
    """The k-mers strictly between u and v on the strongest path, or None where it fails."""
    x, S = u, []
    while True:
        y = strong_step(cnt, K, x, min_cov, min_arc)
        if y is None:
            return None
        if y == v:
            return S
        if T.key_of(y) in (T.key_of(u), T.key_of(v)) or len(S) == most:
            return None
        S.append(y)
        x = y


def decide(cnt, K, min_cov, min_arc, max_len, max_diff):
    """(the minor arms as (u, v, members, S), the arms kept), every arm once: in its deciding orientation."""
    cov = lambda members: sum(B.coverage(cnt[T.key_of(m)]) for m in members)
    minor, kept = [], []
    for u, v, mp in B.branches(cnt, K, min_cov, min_arc, max_len):
        if mp[0][0] > T.flip(mp[-1])[0]:
            continue                                                            # (decided from its other end)
        S = strongest_path(cnt, K, u, v, len(mp) + max_diff, min_cov, min_arc)
        if S and S[0] != mp[0] and abs(len(mp) - len(S)) <= max_diff and cov(mp) * len(S) < cov(S) * len(mp):
            minor.append((u, v, mp, S))
        else:
            kept.append((u, v, mp))
    return minor, kept


def bulge_round(model, min_cov, min_arc, max_len, max_diff):
    """One round on model.cnt, in place: (totals [arms popped, k-mers removed, solid before, arms kept], the set of removed keys, the
    list of (junction key, which half -- 0 low --, which counter of it) cleared)."""
    K, cnt = model.K, model.cnt
    before = dict(cnt)
    n_solid = sum(1 for w in before.values() if T.solid(w, min_cov))
    minor, kept = decide(before, K, min_cov, min_arc, max_len, max_diff)
    removed, cleared = set(), []
    for u, v, members, S in minor:
        keys = [T.key_of(m) for m in members]
        assert not removed & set(keys) and len(set(keys)) == len(keys), "a k-mer lies in two popped arms"
        removed.update(keys)
    for u, v, members, S in minor:
        assert not removed & {T.key_of(s) for s in S}, "a k-mer of a strongest path that justified a pop is removed"
        for y, a in ((v, T.first_base(members[-1], K)), (T.flip(u), T.first_base(T.flip(members[0]), K))):
            half, idx = (0, a) if T.is_fwd(y) else (1, a ^ 2)
            assert T.key_of(y) not in removed, "a junction is a removed key"
            cnt[T.key_of(y)] &= ~(63 << (32 * half + 6 * idx))
            cleared.append((T.key_of(y), half, idx))
    for k in removed:
        cnt[k] = 0
    for u, v, members, S in minor:
        assert strongest_path(cnt, K, u, v, len(S), min_cov, min_arc) == S, "a fork no longer reaches its join by strong steps"
    return [len(minor), len(removed), n_solid, len(kept)], removed, cleared
