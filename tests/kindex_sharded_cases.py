"""The cases of the k-mer index cut over ranks (pg_kindex_build_sharded, pg_kindex_query_words), shared by
tests/test_kindex_sharded_host.py (the host twin, devices all -1) and tests/test_gpu_kindex_sharded.py (every rank on GPU 0).  The
tables, sequences and the comparison with the model are tests/kindex_cases.py's; here are the cut, stated independently of the library
(`owner`), the index under test built over a device tuple, and the designed cuts.  All comparisons are of integers and exact."""
import functools

import numpy as np

import kindex_cases as E
import kindex_model as M
from soapdenovo2_amd import api

RANKS = [1, 2, 3, 8]
WIDE = [(31, False), (65, True)]       # the flavours every rank count of RANKS runs with


def owner(key, nw, n):
    """The rank of n that holds a canonical key: bits 40 and up of the key's hash, modulo n."""
    return (M.key_hash(key, nw) >> 40) % n


def owner_counts(keys, nw, n):
    return [int(c) for c in np.bincount([owner(k, nw, n) for k in keys], minlength=n)]


@functools.lru_cache(maxsize=None)
def budget_table(K, mer127):
    """(records, keys, the sequence they are cut from) of 20 000 distinct keys, none deleted: a table above 1 MB over one rank (65 536
    slots) whatever the flavour."""
    nw = 4 if mer127 else 2
    codes = np.random.default_rng(4242 + K).integers(0, 4, size=21000, dtype=np.uint8)
    keys = list(dict.fromkeys(M.canonical_kmers(codes, K)))[:20000]
    assert len(keys) == 20000
    return E._records(keys, nw, np.random.default_rng(K), deleted=False), keys, codes


class Index(E.Index):
    """kindex_cases.Index over a device tuple: batches and answers lie on the lead (devices[0]); parts = the records as several arrays
    (numpy: host parts; torch tensors: device parts), else `records` is the one part."""

    def __init__(self, records, K, mer127, devices, parts=None):
        self.K, self.mer127, self.devices, self.device = K, mer127, tuple(devices), devices[0]
        self.nw = 4 if mer127 else 2
        self.model = M.Model.from_records(records, K, self.nw)
        self.ix = api.KmerIndex.from_records(records, K, mer127, self.devices) if parts is None else \
            api.KmerIndex.from_parts(parts, K, mer127, self.devices)

    def words(self, seqs, wave=False):
        """Every answer and every summary word of a ragged batch, as one array."""
        cnt, summ, _ = self.ragged(seqs, wave)
        return np.concatenate([cnt, summ.reshape(-1)])


def check_info(ix, keys, nw, devices):
    """Per rank: the keys it owns by the Python statement of the cut, a table of exactly that many; the totals."""
    n = len(devices)
    info = ix.info()
    want = owner_counts(keys, nw, n)
    assert [r["keys"] for r in info["ranks"]] == want and sum(want) == len(keys) == info["keys"]
    assert [r["slots"] for r in info["ranks"]] == [M.table_slots(k) for k in want]
    assert [r["bytes"] for r in info["ranks"]] == [M.table_slots(k) * (nw + 2) * 8 for k in want]
    assert [r["device"] for r in info["ranks"]] == list(devices) and info["device"] == devices[0]
    assert info["slots"] == sum(r["slots"] for r in info["ranks"]) and info["bytes"] == sum(r["bytes"] for r in info["ranks"])
    if n == 1:                                                                # a one-rank cut is pg_kindex_build's table
        assert (info["keys"], info["slots"], info["bytes"]) == (len(keys), M.table_slots(len(keys)), api.host_kindex_bytes(len(keys), nw == 4))


def check_table(name, K, mer127, devices, waves=(False,)):
    """kindex_cases.check_table for an index over `devices`: one table against the model on every batch of the list."""
    records, keys = E.table(name, K, mer127)
    seqs, tags = E.sequences(K)
    ix = Index(records, K, mer127, devices)
    try:
        check_info(ix.ix, keys, ix.nw, devices)
        for wave in waves:
            what = "%s %s over %d ranks wave=%s" % (name, E.flavour_id((K, mer127)), len(devices), wave)
            cnt, summ = ix.check_ragged(seqs, wave, what)
            if name == "empty":
                assert not cnt.any() and not summ[:, :3].any()
            if keys and name != "colliding":                                  # the first record's value bit for bit
                first = ix.model.cnt[keys[0]]
                assert first >> 63 == 1 and first in [int(c) for c in cnt]
            ix.check_ragged([], wave, what + " no sequences")
            ix.check_ragged([s for s in seqs if len(s) < K], wave, what + " no k-mers")
            for L in (K - 1, K, K + 1, 2 * K + 1):
                batch = [s for s in seqs if len(s) == L]
                u_cnt, u_summ = ix.uniform(np.stack(batch), wave)
                w_cnt, w_summ = ix.want(batch)
                assert (u_cnt == w_cnt).all() and (u_summ == w_summ).all(), what + " uniform %d" % L
    finally:
        ix.close()


# The designed cuts are what they are named for: `one` over 8 ranks leaves seven ranks without a key, and the genome's keys reach every
# rank of 2, 3 and 8 -- so a rank without keys, and every rank's own table, are both looked into
for _K, _mer127 in E.FLAVOURS:
    _nw = 4 if _mer127 else 2
    assert sorted(owner_counts(E.table("one", _K, _mer127)[1], _nw, 8)) == [0] * 7 + [1]
    for _n in (2, 3, 8):
        assert min(owner_counts(E.table("genome", _K, _mer127)[1], _nw, _n)) >= 1
# and the budget test's table is above the 1 MB its hook allows over one rank, in the flavour it runs in (the genome's table there is not)
assert M.table_slots(len(E.table("genome", 65, True)[1])) * 48 < 1 << 20 < M.table_slots(len(budget_table(65, True)[1])) * 48
