// p2_walk.hpp -- parse1read (prlRead2path.c:598-745) once, for the device kernels (p2_kernels.hpp) and the host twin
// (host_graph.cpp: ReadThreader): the state machine that turns the node words of a read's k-mers, in read order, into edge
// ids, the pre-arcs between them and the -R walk.  Host + device (PG_HD), no device-only types.
// The caller supplies a sink: kplus(canonical (K+1)-mer, smaller) -> the id of its length-1 edge in the patch map, 0 = not there (search1kmerPlus,
// prlRead2path.c:558-596); pair(from, to, i), one pre-arc, i = index of `from` among the read's items (thread_add1preArc, :224-254); item(i, id), item i of
// the read (the -R row; a restart begins again at 0).
#pragma once
#include <stdint.h>

#include "kmer.hpp"

namespace pg {

template <int NW>
struct P2Walk {
    unsigned retain = 0;
    bool is_prev = false, stop = false;
    Kmer<NW> prev_k;
    int n_items = 0;             // items pushed since the last restart
    int n_valid = -1;            // index of the first unresolved item (id 0), -1 while there is none
    uint32_t last_id = 0;        // id of the latest item
    PG_HD P2Walk() {
#pragma unroll
        for (int i = 0; i < NW; i++) prev_k.w[i] = 0;
    }
};

// one k-mer of the read: `canon` its canonical form, `smaller` = the read spells it, `ab` = its node's two words.  w.stop afterwards: the read is over
template <int NW, typename Sink>
PG_HD void p2_walk_step(P2Walk<NW>& w, const Kmer<NW>& canon, bool smaller, uint64_t ab, int K, Sink& sink) {
    const uint32_t A = (uint32_t)ab, B = (uint32_t)(ab >> 32);
    const bool linear = B & B_LINEAR, in_edge = (B >> B_INEDGE_SHIFT) & 3;
    if ((B & B_DELETED) || (linear && !in_edge)) {                   // deleted, or on a floating loop
        // a restart forgets the items, NOT is_prev / prev_k: they keep their stale values, as the reference's locals do
        if (w.retain < 2) { w.retain = 0; w.n_items = 0; w.n_valid = -1; }
        else w.stop = true;
        return;
    }
    uint32_t id = 0;
    bool push = false;
    if (linear) {
        const uint32_t twin = (B >> B_TWIN_SHIFT) & 3;
        id = smaller ? A : A + twin - 1;
        if (w.retain == 0 || w.is_prev) { push = true; w.is_prev = false; }
        else if (id != w.last_id) push = true;
    } else {
        const Kmer<NW> wq = smaller ? canon : kmer_rc<NW>(canon, K);    // the k-mer as the read spells it (prlRead2path.c:680-687)
        if (w.is_prev) {                                             // branch node after branch node: a length-1 edge
            // The reference resolves the (K+1)-mers of a read after parse1read, and only when two items were retained; here it is done on the spot.  No result
            // can tell: the one comparison with the previous item's id (`id != w.last_id` above) is not reached while is_prev is set.
            const Kmer<NW> plus = kmer_plus<NW>(w.prev_k, kmer_last<NW>(wq));
            const Kmer<NW> bal_plus = rc_plus<NW>(plus, K);
            const bool sm = kmer_less<NW>(plus, bal_plus);
            id = sink.kplus(sm ? plus : bal_plus, sm);
            push = true;
        }
        w.is_prev = true;
        w.prev_k = wq;
    }
    if (!push) return;
    w.retain++;
    // the pre-arcs are the items pairwise up to the first unresolved one; an item is never taken back once two are retained, so a pair goes out with its second half
    if (w.n_items >= 1 && w.n_valid < 0 && id != 0) sink.pair(w.last_id, id, w.n_items - 1);
    if (id == 0 && w.n_valid < 0) w.n_valid = w.n_items;
    sink.item(w.n_items, id);
    w.last_id = id;
    w.n_items++;
}

// the read is through (prlRead2path.c:723-733, recordPathBin :478-543)
struct P2WalkEnd {
    bool deleted;                // no usable item at all: the reference's "read(s) deleted" counter
    int walk;                    // entries of the -R walk, up to the first unresolved one; 0 unless two items were retained and the first three are resolved
};
template <int NW>
PG_HD P2WalkEnd p2_walk_end(const P2Walk<NW>& w) {
    P2WalkEnd e{w.retain < 1, 0};
    if (w.retain < 2) return e;
    const int upto = w.n_valid < 0 ? w.n_items : w.n_valid;
    if (upto >= 3) e.walk = upto;
    return e;
}

}  // namespace pg
