"""An independent model of bubble popping (include/soapdenovo2_amd.h, pg_kindex_pop_bubbles), written from the rule and sharing no code
with the library: the index is kindex_model.Model's dict from canonical k-mer (a Python int) to cnt word, which a round changes in place;
an oriented k-mer is ktip_model's pair (its value, its reverse complement's value) of Python ints, and the side test is ktip_model.side.
Where the library decides a branch from one of its starts and looks for its siblings behind the fork, the model lists every branch of
the graph in both orientations first and groups them by their junctions.

  * a branch: an oriented solid k-mer x0 whose left side is BRANCH_IN -- L the k-mer behind it, as the step from rc(x0) reaches it --,
    to the right through open sides, at most max_len k-mers, to a side that ends with BRANCH_IN -- v the k-mer behind it --, and
    canon(L) != canon(v).  u = rc(L) is the fork
  * siblings: two branches with the same oriented u and the same oriented v whose lengths differ by at most max_diff, and the arc from
    u to the sibling's first k-mer exists (its out-counter in u's word is >= min_arc)
  * minor: some sibling Q has cov_P * n_Q < cov_Q * n_P, cov the sum of the members' coverage.  A branch is decided in the orientation
    whose first k-mer is not greater than the reverse complement of its last
  * a round decides every branch on the dict as it stood, then applies: every k-mer of a minor branch gets the word 0, in v's word the
    in-counter for the first base of the last k-mer becomes 0, and in L's word the in-counter for the first base of rc(x0)

pop_round() asserts for itself that no junction is a removed key, that no k-mer lies in two popped branches and that every bubble keeps
a branch."""
import ktip_model as T

BRANCH_IN, TOO_LONG = T.BRANCH_IN, T.TOO_LONG


def coverage(w):
    return (w >> 24) & 0xFF


def walk(cnt, K, x0, min_cov, min_arc, max_len):
    """From the solid oriented k-mer x0 to the right through open sides: (members, the reason of the side that ended it, the k-mer behind)."""
    members = [x0]
    while True:
        reason, y = T.side(cnt, K, members[-1], min_cov, min_arc)
        if not reason and len(members) == max_len:
            reason = TOO_LONG
        if reason:
            return members, reason, y
        members.append(y)


_RC4 = [sum((((b >> 2 * i) & 3) ^ 2) << 2 * (3 - i) for i in range(4)) for b in range(256)]     # the reverse complement of four bases


def node_of_key(key, K):
    """ktip_model.node_of_key, four bases at a time: (value, value of the reverse complement).  The key is padded with A's behind it to
    whole bytes; their complements come out in front and are cut off."""
    pad = -K % 4
    r = int.from_bytes(bytes(_RC4[b] for b in (key << 2 * pad).to_bytes((K + pad) // 4, "little")), "big")
    return key, r & ((1 << 2 * K) - 1)


def branches(cnt, K, min_cov, min_arc, max_len):
    """Every branch of the dict, in both of its orientations, as (u, v, members)."""
    out = []
    for key in sorted(k for k, w in cnt.items() if T.solid(w, min_cov)):
        x = node_of_key(key, K)
        for x0 in (x, T.flip(x)):
            reason, L = T.side(cnt, K, T.flip(x0), min_cov, min_arc)
            if reason != BRANCH_IN:
                continue
            members, reason, v = walk(cnt, K, x0, min_cov, min_arc, max_len)
            if reason == BRANCH_IN and T.key_of(L) != T.key_of(v):
                out.append((T.flip(L), v, members))
    return out


def decide(cnt, K, min_cov, min_arc, max_len, max_diff):
    """(the minor branches, the branches kept, the bubbles as lists of branches), every branch once: in its deciding orientation."""
    groups = {}
    for b in branches(cnt, K, min_cov, min_arc, max_len):
        groups.setdefault((b[0], b[1]), []).append(b)
    cov = lambda members: sum(coverage(cnt[T.key_of(m)]) for m in members)
    minor, kept = [], []
    for (u, v), group in groups.items():
        arcs_out = T.out_counters(cnt[T.key_of(u)], T.is_fwd(u))
        for P in group:
            mp = P[2]
            if mp[0][0] > T.flip(mp[-1])[0]:
                continue                                                        # (decided from its other end)
            weaker = False
            for Q in group:
                mq = Q[2]
                if Q is P or abs(len(mp) - len(mq)) > max_diff or arcs_out[mq[0][0] & 3] < min_arc:
                    continue
                weaker = weaker or cov(mp) * len(mq) < cov(mq) * len(mp)
            (minor if weaker else kept).append(P)
    return minor, kept, list(groups.values())


def pop_round(model, min_cov, min_arc, max_len, max_diff):
    """One round on model.cnt, in place: (totals [branches, k-mers removed, solid before, candidates kept], the set of removed keys, the
    list of (junction key, which half -- 0 low --, which counter of it) cleared)."""
    K, cnt = model.K, model.cnt
    before = dict(cnt)
    n_solid = sum(1 for w in before.values() if T.solid(w, min_cov))
    minor, kept, bubbles = decide(before, K, min_cov, min_arc, max_len, max_diff)
    removed, cleared = set(), []
    for u, v, members in minor:
        keys = [T.key_of(m) for m in members]
        assert not removed & set(keys) and len(set(keys)) == len(keys), "a k-mer lies in two popped branches"
        removed.update(keys)
    gone = {frozenset(T.key_of(m) for m in members) for _, _, members in minor}
    for group in bubbles:
        if any(frozenset(T.key_of(m) for m in members) in gone for _, _, members in group):
            assert any(frozenset(T.key_of(m) for m in members) not in gone for _, _, members in group), "a bubble keeps no branch"
    for u, v, members in minor:
        for y, a in ((v, T.first_base(members[-1], K)), (T.flip(u), T.first_base(T.flip(members[0]), K))):
            half, idx = (0, a) if T.is_fwd(y) else (1, a ^ 2)
            assert T.key_of(y) not in removed, "a junction is a removed key"
            cnt[T.key_of(y)] &= ~(63 << (32 * half + 6 * idx))
            cleared.append((T.key_of(y), half, idx))
    for k in removed:
        cnt[k] = 0
    return [len(minor), len(removed), n_solid, len(kept)], removed, cleared
