"""An independent model of the read corrector (include/soapdenovo2_amd.h, pg_kindex_correct), written from the rule and sharing no code
with the library: reads are lists of base codes (A0 C1 T2 G3), the index is kindex_model.Model's dict, a k-mer is looked up by building
its integer from the K codes -- no packed words, nothing rolls.

  * a read of L bases has nk = max(0, L - K + 1) k-mers; k-mer j is bases [j, j + K)
  * solid(j): the model's answer for the canonical k-mer j of the read as it currently stands is not 0 and its coverage is >= min_cov
  * anchor s = the first solid k-mer of the read as given; nk == 0 -> NO_KMERS, none solid -> NO_ANCHOR, the read is returned as it is
  * right sweep j = s + 1 .. nk - 1, then left sweep j = s - 1 .. 0: a solid k-mer is passed; at a weak one, with fixes == max_fixes the
    sweep ends with LIMIT; else base p (right: j + K - 1, left: j) goes on trial
  * trial: for each x != read[p], ext(x) = consecutive solid k-mers from j on in the sweep's direction among the k-mers that hold p
    (right: j .. min(p, nk - 1), left: j .. max(0, p - K + 1); `full` of them), with p replaced by x.  Accepted for x* iff
    ext(x*) >= min(min_run, full) and ext(x*) > ext(x) for both other x: the base is written and fixes += 1.  Else the sweep ends with
    STOP_RIGHT / STOP_LEFT and nothing is written
  * report = fixes | flags | (weak k-mers of the read as given) << 32"""
import kindex_model as M

NO_KMERS, NO_ANCHOR, STOP_RIGHT, STOP_LEFT, LIMIT = 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12


def kmer_at(read, j, K):
    """The canonical k-mer of bases [j, j + K) as an int."""
    fwd = rev = 0
    for c in read[j:j + K]:
        fwd = fwd << 2 | c
    for c in reversed(read[j:j + K]):
        rev = rev << 2 | (c ^ 2)
    return min(fwd, rev)


def solid(model, read, j, min_cov):
    cnt = model.cnt.get(kmer_at(read, j, model.K), 0)
    return cnt != 0 and M.coverage(cnt) >= min_cov


def correct(model, codes, min_cov, max_fixes, min_run):
    """(the corrected read as a list of codes, the report word)."""
    K = model.K
    read = [int(c) & 3 for c in codes]
    nk = max(0, len(read) - K + 1)
    if nk == 0:
        return read, NO_KMERS
    given = [solid(model, read, j, min_cov) for j in range(nk)]
    weak = given.count(False) << 32
    if True not in given:
        return read, NO_ANCHOR | weak
    s = given.index(True)
    fixes, flags = 0, 0
    for step, stop_flag, order in ((1, STOP_RIGHT, range(s + 1, nk)), (-1, STOP_LEFT, range(s - 1, -1, -1))):
        for j in order:
            if solid(model, read, j, min_cov):
                continue
            if fixes == max_fixes:
                flags |= LIMIT
                break
            p = j + K - 1 if step > 0 else j
            holders = list(range(j, min(p, nk - 1) + 1)) if step > 0 else list(range(j, max(0, p - K + 1) - 1, -1))
            ext = {}
            for x in range(4):
                if x == read[p]:
                    continue
                trial = list(read)
                trial[p] = x
                n = 0
                for h in holders:
                    if not solid(model, trial, h, min_cov):
                        break
                    n += 1
                ext[x] = n
            best = max(ext, key=lambda x: ext[x])
            if ext[best] >= min(min_run, len(holders)) and all(ext[best] > ext[x] for x in ext if x != best):
                read[p] = best
                fixes += 1
            else:
                flags |= stop_flag
                break
    return read, fixes | flags | weak
