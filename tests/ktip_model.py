"""An independent model of tip clipping (include/soapdenovo2_amd.h, pg_kindex_clip_tips), written from the rule and sharing no code with
the library: the index is kindex_model.Model's dict from canonical k-mer (a Python int) to cnt word, which a round changes in place; an
oriented k-mer is the pair (its value, its reverse complement's value) of Python ints, stepped by arithmetic on those, never packed
words or table slots.

  * the cnt word of a canonical k-mer: left counter a = bits 6a+5:6a of its low half, right counter b the same bits of its high half,
    coverage = bits 31:24.  For an oriented k-mer x with canonical form c: x == c: out(b) = right[b], in(a) = left[a]; x == rc(c):
    out(b) = left[b ^ 2], in(a) = right[a ^ 2]
  * solid = a word that is not 0 with coverage >= min_cov; an arc exists when its counter is >= min_arc
  * the right side of a solid oriented k-mer x is open when exactly one arc b leaves it, y = x[1:] + [b] is solid, the arcs into y are
    exactly [x[0]] and canon(y) != canon(x); otherwise it is an end: DEAD_END (no arc out), BRANCH_OUT (several), WEAK_NEXT, BRANCH_IN,
    HAIRPIN, the first that applies.  The left side of x is the right side of rc(x)
  * a tip candidate: from an oriented solid k-mer whose left side is DEAD_END or WEAK_NEXT, to the right through open sides, at most
    max_tip k-mers, to a side that ends with BRANCH_IN.  y = the k-mer behind that side, a = the first base of the last k-mer
  * minor: y's raw in-counter for a is strictly smaller than the largest of y's other three in-counters
  * a round decides every candidate on the dict as it stood, then applies: every k-mer of a minor tip gets the word 0, and in y's word the
    one in-counter for a becomes 0

clip_round() asserts for itself that no junction is a removed key and that no k-mer lies in two tips."""
DEAD_END, BRANCH_OUT, WEAK_NEXT, BRANCH_IN, HAIRPIN, TOO_LONG = 3, 4, 5, 6, 9, 11


def node_of_key(key, K):
    """The canonical k-mer as an oriented one: (value, value of the reverse complement)."""
    r = 0
    for i in range(K):
        r = (r << 2) | (((key >> 2 * i) & 3) ^ 2)
    return key, r


def flip(x):
    return x[1], x[0]


def step(x, b, K):
    return ((x[0] << 2) | b) & ((1 << 2 * K) - 1), (x[1] >> 2) | ((b ^ 2) << 2 * (K - 1))


def key_of(x):
    return min(x)


def is_fwd(x):
    return x[0] <= x[1]


def first_base(x, K):
    return x[0] >> 2 * (K - 1)


def out_counters(w, fwd):
    return [(w >> 32 >> 6 * b) & 63 if fwd else (w >> 6 * (b ^ 2)) & 63 for b in range(4)]


def in_counters(w, fwd):
    return [(w >> 6 * a) & 63 if fwd else (w >> 32 >> 6 * (a ^ 2)) & 63 for a in range(4)]


def solid(w, min_cov):
    return w != 0 and (w >> 24) & 0xFF >= min_cov


def side(cnt, K, x, min_cov, min_arc):
    """The right side of the solid oriented k-mer x: (0, y) when it is open; (reason, y) when it is an end -- y the k-mer behind it where
    the reason is WEAK_NEXT, BRANCH_IN or HAIRPIN, else None."""
    nxt = [b for b, n in enumerate(out_counters(cnt[key_of(x)], is_fwd(x))) if n >= min_arc]
    if not nxt:
        return DEAD_END, None
    if len(nxt) > 1:
        return BRANCH_OUT, None
    y = step(x, nxt[0], K)
    wy = cnt.get(key_of(y), 0)
    if not solid(wy, min_cov):
        return WEAK_NEXT, y
    if [a for a, n in enumerate(in_counters(wy, is_fwd(y))) if n >= min_arc] != [first_base(x, K)]:
        return BRANCH_IN, y
    if key_of(y) == key_of(x):
        return HAIRPIN, y
    return 0, y


def is_minor(cnt, K, last, y):
    """The minor test for a tip whose last k-mer is `last` and whose junction is y."""
    a = first_base(last, K)
    ins = in_counters(cnt[key_of(y)], is_fwd(y))
    return ins[a] < max(n for c, n in enumerate(ins) if c != a)


def candidates(cnt, K, min_cov, min_arc, max_tip):
    """Every tip candidate of the dict as (member keys from the free end on, the last k-mer, the junction)."""
    out = []
    for key in sorted(k for k, w in cnt.items() if solid(w, min_cov)):
        for x0 in (node_of_key(key, K), flip(node_of_key(key, K))):
            if side(cnt, K, flip(x0), min_cov, min_arc)[0] not in (DEAD_END, WEAK_NEXT):
                continue
            x, members = x0, [key]
            while True:
                reason, y = side(cnt, K, x, min_cov, min_arc)
                if not reason and len(members) == max_tip:
                    reason = TOO_LONG
                if reason:
                    break
                members.append(key_of(y))
                x = y
            if reason == BRANCH_IN:
                out.append((members, x, y))
    return out


def clip_round(model, min_cov, min_arc, max_tip):
    """One round on model.cnt, in place: (totals [tips, k-mers removed, solid before, candidates kept], the set of removed keys, the
    list of (junction key, which half -- 0 low --, which counter of it) cleared)."""
    K, cnt = model.K, model.cnt
    before = dict(cnt)
    n_solid = sum(1 for w in before.values() if solid(w, min_cov))
    tips, kept = [], 0
    for members, last, y in candidates(before, K, min_cov, min_arc, max_tip):
        if is_minor(before, K, last, y):
            tips.append((members, last, y))
        else:
            kept += 1
    removed, cleared = set(), []
    for members, last, y in tips:
        assert not removed & set(members) and len(set(members)) == len(members), "a k-mer lies in two tips"
        removed.update(members)
    for members, last, y in tips:
        a = first_base(last, K)
        half, idx = (0, a) if is_fwd(y) else (1, a ^ 2)
        assert key_of(y) not in removed, "a junction is a removed key"
        cnt[key_of(y)] &= ~(63 << (32 * half + 6 * idx))
        cleared.append((key_of(y), half, idx))
    for k in removed:
        cnt[k] = 0
    return [len(tips), len(removed), n_solid, kept], removed, cleared
