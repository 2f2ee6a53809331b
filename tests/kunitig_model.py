"""An independent model of the unitigs (include/soapdenovo2_amd.h, pg_kindex_unitigs), written from the rule and sharing no code with the
library: the index is kindex_model.Model's dict from canonical k-mer (a Python int) to cnt word, and everything steps over lists of base
codes, never packed words or table slots.  The arc decoding is kwalk_model's (itself written from the definitions).

  * solid = in the set (not deleted) with coverage >= min_cov; an arc exists when its counter is >= min_arc
  * the right side of a solid oriented k-mer x is open when exactly one arc b leaves it, y = x[1:] + [b] is solid, the arcs into y are
    exactly [x[0]] and canon(y) != canon(x); otherwise it is an end: DEAD_END (no arc out), BRANCH_OUT (several), WEAK_NEXT, BRANCH_IN,
    HAIRPIN, the first that applies.  The left side of x is the right side of rc(x), and its reason is the unitig's left reason
  * a linear unitig: from every oriented solid k-mer whose left side is an end, to the right through open sides to an end; text = the
    first k-mer and the appended bases.  Found from both ends; the copy whose first k-mer is not greater (as an integer) is kept
  * a ring: solid k-mers that no chain reaches; kept once, from the member with the least canonical k-mer, as that k-mer reads, to the
    right, both reasons CYCLE
  * max_kmers: a chain stops there with CUT on the right and both copies are kept; a ring of more k-mers is not emitted

unitigs() returns the LIST of (text, left reason, right reason, coverage sum), texts as tuples; the tests compare it sorted and check that
it holds nothing twice."""
import kindex_model as M
import kwalk_model as W

DEAD_END, BRANCH_OUT, WEAK_NEXT, BRANCH_IN = W.DEAD_END, W.BRANCH_OUT, W.WEAK_NEXT, W.BRANCH_IN
HAIRPIN, CYCLE, CUT = 9, 10, 11
NAMES = {DEAD_END: "dead_end", BRANCH_OUT: "branch_out", WEAK_NEXT: "weak_next", BRANCH_IN: "branch_in", HAIRPIN: "hairpin", CYCLE: "cycle", CUT: "cut"}


def codes_of(key, K):
    return [(key >> 2 * (K - 1 - i)) & 3 for i in range(K)]


def side(model, x, min_cov, min_arc):
    """The right side of the solid oriented k-mer x: (0, y) when it is open, (reason, None) when it is an end."""
    key, fwd = W.oriented(x)
    nxt = [b for b, n in enumerate(W.out_arcs(model.cnt[key], fwd)) if n >= min_arc]
    if not nxt:
        return DEAD_END, None
    if len(nxt) > 1:
        return BRANCH_OUT, None
    y = x[1:] + nxt
    ykey, yfwd = W.oriented(y)
    wy = model.cnt.get(ykey, 0)
    if not W.solid(wy, min_cov):
        return WEAK_NEXT, None
    if [a for a, n in enumerate(W.in_arcs(wy, yfwd)) if n >= min_arc] != [x[0]]:
        return BRANCH_IN, None
    if ykey == key:
        return HAIRPIN, None
    return 0, y


def solid_keys(model, min_cov):
    return sorted(k for k, w in model.cnt.items() if W.solid(w, min_cov))


def unitigs(model, min_cov, min_arc, max_kmers=1 << 24):
    """(the list of (text, left, right, coverage sum), the number of cut unitigs)."""
    K = model.K
    out, covered, n_cut = [], set(), 0
    keys = solid_keys(model, min_cov)
    for key in keys:
        c = codes_of(key, K)
        for x0 in (c, W.revcomp(c)):
            left, _ = side(model, W.revcomp(x0), min_cov, min_arc)
            if not left:
                continue
            x, text, seen, cov = x0, list(x0), [W.oriented(x0)[0]], M.coverage(model.cnt[key])
            while True:
                right, y = side(model, x, min_cov, min_arc)
                if not right and len(seen) == max_kmers:
                    right = CUT
                if right:
                    break
                text.append(y[-1])
                seen.append(W.oriented(y)[0])
                cov += M.coverage(model.cnt[seen[-1]])
                x = y
            assert len(set(seen)) == len(seen), "a chain from an end met a canonical k-mer twice"
            covered.update(seen)
            if right == CUT:
                n_cut += 1
            elif W.value(W.revcomp(x)) < W.value(x0):
                continue
            out.append((tuple(text), left, right, cov))
    in_ring = set()
    for key in keys:
        if key in covered or key in in_ring:
            continue
        # to the right through open sides: back to the start (a ring), or to an end or a covered k-mer (the inside of a cut chain)
        x, members, ring = codes_of(key, K), [key], None
        while ring is None:
            reason, y = side(model, x, min_cov, min_arc)
            if reason or W.oriented(y)[0] in covered:
                ring = False
            elif W.oriented(y)[0] == key:
                ring = True
            else:
                members.append(W.oriented(y)[0])
                x = y
                assert len(members) <= len(keys)
        if not ring:
            continue
        assert len(set(members)) == len(members)
        in_ring.update(members)
        if len(members) > max_kmers:
            continue
        x = codes_of(min(members), K)
        text, cov = list(x), 0
        for i in range(len(members)):
            cov += M.coverage(model.cnt[W.oriented(x)[0]])
            reason, y = side(model, x, min_cov, min_arc)
            assert not reason
            if i + 1 < len(members):
                text.append(y[-1])
            x = y
        assert W.oriented(x)[0] == min(members)
        out.append((tuple(text), CYCLE, CYCLE, cov))
    return out, n_cut


def kmers_of(text, K):
    """The canonical k-mers of a unitig's text."""
    return M.canonical_kmers(list(text), K)
