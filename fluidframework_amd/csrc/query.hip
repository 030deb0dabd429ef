// query.hip -- batched position queries (mtr_get_containing_segments): many (document, pos, refSeq, client) views
// answered in one launch, with the segments' text and properties gathered on the device.
//
// Three kernels on the engine stream, none of them an apply kernel (the launch census does not count them):
//   containing_batch_kernel  one workgroup (one wave) per query: Eng<true>::containing with the query's own parameters,
//                            its 11 result words to row i; lane 0 then derives the query's two lengths from the row
//                            (text units, property words; none for a matrix vector, none for a half the caller
//                            skips) with mtr_get_props' bounds checks
//   query_scan_kernel        64-bit exclusive scans of both length arrays, totals last (delta_scan_kernel's scheme)
//   query_gather_kernel      one wave per query copies its text units and its property words into two compact buffers
// The host uploads the queries once and downloads the rows, the offsets (both arrays and the error flag in one copy),
// then the text and the properties: four device-to-host copies and two synchronisations for any n.
//
// Batched reference queries (mtr_get_refs): the local references of many documents in one launch, in the words of
// mtr_get_ref_positions / _states / _keys.
//   refs_count_kernel        one lane per listed document: its references (DocHdr.nrefs) and its 64-reference blocks
//   query_scan_kernel        (the same kernel) scans both, totals last, the corrupted-header flag carried along
//   refs_work_kernel         one lane per listed document writes its blocks' (listed index, block) work items
//   refs_batch_kernel        one workgroup (one wave) per work item: one 64-reference round of Eng<true>::ref_query
// The host uploads the list once (not at all for documents 0 .. n - 1) and downloads doc_first with the block total
// and the flag in one copy, then the words: two device-to-host copies and two synchronisations for any n.
//
// Batched range queries (mtr_get_range_segments): the segments, the text and the properties of many ranges [start, end),
// each at its own view -- the walk of mtr_get_containing_segment over a range, for many ranges in two launches.
//   range_count_kernel       one workgroup (one wave) per query: its segments, clipped text units and property words,
//                            counted in rounds of 64 leaves; the round its first segment is in
//   range_scan_kernel        query_scan_kernel's scheme for the three count arrays, totals last, the flag carried along
//   range_write_kernel       one wave per query, from that round: the segments' rows and offsets, their units and words
// The host uploads the queries once and downloads the three scans with the flag in one copy, then what the caller asked
// for (rows, two offset arrays, text, properties): at most six device-to-host copies and two synchronisations.
//
// Batched delta records (mtr_get_deltas_batch): the delta records of many documents, in mtr_get_deltas' fields, with the
// property sets mtr_get_props returns for their MTR_DELTA_REGEN_X records.
//   delta_count_kernel       one wave per listed document: its records (DocHdr.dused, checked against its slice) and
//                            the property words of its records, read 64 records a round
//   query_scan_kernel        (the same kernel) scans both, totals last, the flag carried along
//   delta_records_kernel     one wave per listed document: its records as 16-byte units, each record's offset into the
//                            words, the property sets copied 64 lanes wide
// The host uploads the list once (not at all for documents 0 .. n - 1) and downloads doc_first with the word total and
// the flag in one copy, then the records, the offsets and the words: at most four device-to-host copies and two
// synchronisations for any n.
//
// Batched position transforms (mtr_transform_positions): positions of one view, or leaf ordinals, mapped into another
// view of the same document -- Client.resolveRemoteClientPosition and Client.getPosition for many (document, view) pairs.
//   position_kernel          one workgroup (one wave) per query: both views of the same leaves evaluated in one walk
//                            of rounds of 64, the walk left in the round that finds the leaf; one 16-byte row a query
// The host uploads the queries once and downloads the rows: one device-to-host copy and one synchronisation for any n.
//
// Batched interval queries (mtr_query_intervals): findOverlappingIntervals, previousInterval and nextInterval of many
// interval collections of many documents, over the compare keys of the collections' endpoint references.
//   interval_keys_kernel     one wave per 32 intervals of a set: ref_query's key round for those 64 endpoints alone
//   interval_count_kernel    one wave per query: the keys of its positions in the local view from one walk of the
//                            leaves, then the set's intervals 64 a round: its hits, its status, its work row
//   query_scan_kernel        (the same kernel) scans the hits and the status words, the flag carried along
//   interval_write_kernel    one wave per query: the hits' 32-byte rows at their places
// The host uploads the sets, the queries, the keys kernel's work list and the reference ids in one copy and downloads
// hit_first, the status words and the flag in one copy, then the rows: two synchronisations for any n.
//
// Batched marker search (mtr_find_markers): SharedString.findTile and getMarkerFromId + getPosition for many (document,
// view) pairs -- the marker nearest a position that carries a label, or the marker an id's ordinal is mapped to.
//   marker_find_kernel       one workgroup (one wave) per query: one walk of the leaves at the query's view in rounds
//                            of 64; the property sets of the round's visible markers alone are read, behind one ballot;
//                            one 24-byte row a query
// The host uploads the labels, their value ids and the queries in one copy from page-locked memory and downloads the
// rows with the flag in one copy: one synchronisation for any n.
//
// The unit includes apply.hip.h for Eng<true>::containing, ::ref_query, ::mk_look and the view_open / view_round /
// leaf_row pieces alone; the decoding of a result row is here too (segment_info_from_row), shared with mtr_get_containing_segment.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mtr.h"
#include "apply.hip.h"
#include "engine.hip.h"

using namespace mtr;

namespace {

constexpr int kRowWords = 11;  // Eng::containing's out[0 .. 10]
// bits of the device flag
constexpr int kBadProps = 1;  // a properties reference outside the document's property arena
constexpr int kBadText = 2;   // a text segment outside the document's text arena
// the halves of a call (containing_batch_kernel)
constexpr int kTextHalf = 1, kPropsHalf = 2;

// Row i = Eng<true>::containing of query i.  tlen[i] = the units mtr_get_containing_segment copies for that row (a text
// segment: not a marker), plen[i] = the words mtr_get_props returns for out[8] (1 + 2 n; 0 when the segment has no
// property set or there is no segment).  A matrix vector's segment has neither: it holds no text, and its out[8] is a
// tracking id, whose arena word is a group bit set and no count.  halves: kTextHalf | kPropsHalf, the halves the
// caller asked for; a half that is skipped is neither measured nor checked.
__global__ void __launch_bounds__(NT)
containing_batch_kernel(KParams P, const mtr_view_query* __restrict__ q, const uint32_t* __restrict__ dkind, int halves,
                        int32_t* rows, uint64_t* __restrict__ tlen, uint64_t* __restrict__ plen, int32_t* flag) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t i = blockIdx.x;
    const mtr_view_query x = q[i];
    int32_t* out = rows + size_t(kRowWords) * i;
    Eng<true>::containing(smem, P, x.doc, x.pos, x.ref_seq, x.client, out);
    if (threadIdx.x != 0 || halves == 0) return;  // (lane 0 wrote the row)
    uint64_t t = 0, p = 0;
    if (out[0] >= 0 && dkind[x.doc] == 0) {
        const int len = out[2];
        if ((halves & kTextHalf) && !out[6] && len > 0) {
            if (uint64_t(uint32_t(out[7])) + uint64_t(len) <= uint64_t(P.tcap)) t = uint64_t(len);
            else atomicOr(flag, kBadText);
        }
        if ((halves & kPropsHalf) && out[8] != -1) {
            const uint64_t ref = uint32_t(out[8]), pw = uint64_t(P.pcap);
            if (ref >= pw) {
                atomicOr(flag, kBadProps);
            } else {
                const uint64_t words = 1 + 2 * uint64_t(P.prop[size_t(x.doc) * pw + ref]);
                if (ref + words <= pw) p = words;
                else atomicOr(flag, kBadProps);
            }
        }
    }
    tlen[i] = t;
    plen[i] = p;
}

// off[0 .. n] = the exclusive scan of tlen with its total, off[n + 1 .. 2 n + 1] the same of plen, off[2 n + 2] = the
// flag: one workgroup, a contiguous chunk per thread, as delta_scan_kernel scans the changed lengths.
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads)
query_scan_kernel(const uint64_t* __restrict__ tlen, const uint64_t* __restrict__ plen, uint32_t n,
                  const int32_t* __restrict__ flag, int64_t* __restrict__ off) {
    __shared__ uint64_t tpart[kScanThreads];
    __shared__ uint64_t ppart[kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = uint32_t(min(uint64_t(n), uint64_t(t) * chunk)), hi = uint32_t(min(uint64_t(n), uint64_t(lo) + chunk));
    uint64_t ts = 0, ps = 0;
    for (uint32_t i = lo; i < hi; i++) {
        ts += tlen[i];
        ps += plen[i];
    }
    tpart[t] = ts;
    ppart[t] = ps;
    __syncthreads();
    for (uint32_t step = 1; step < kScanThreads; step <<= 1) {
        const uint64_t a = t >= step ? tpart[t - step] : 0;
        const uint64_t b = t >= step ? ppart[t - step] : 0;
        __syncthreads();
        tpart[t] += a;
        ppart[t] += b;
        __syncthreads();
    }
    uint64_t trun = tpart[t] - ts, prun = ppart[t] - ps;
    int64_t* __restrict__ toff = off;
    int64_t* __restrict__ poff = off + size_t(n) + 1;
    for (uint32_t i = lo; i < hi; i++) {
        toff[i] = int64_t(trun);
        poff[i] = int64_t(prun);
        trun += tlen[i];
        prun += plen[i];
    }
    if (t == kScanThreads - 1) {
        toff[n] = int64_t(tpart[t]);
        poff[n] = int64_t(ppart[t]);
        off[2 * size_t(n) + 2] = *flag;
    }
}

// One wave per query: its text units from the document's text arena (at out[7]) and its property words from the
// property arena (at out[8]) to their offsets in the compact buffers.  Unit by unit and word by word: the copies are
// short, and a text offset that is odd in bytes needs nothing more.  A null destination skips that half.  Every length
// here passed containing_batch_kernel's bounds checks, so every read lies inside the document's arenas; the writes end
// at the totals the host sized the buffers by.
constexpr int kGatherThreads = 256;
__global__ void __launch_bounds__(kGatherThreads)
query_gather_kernel(const mtr_view_query* __restrict__ q, const int32_t* __restrict__ rows,
                    const int64_t* __restrict__ off, uint32_t n, const uint16_t* __restrict__ text, uint32_t tcap,
                    const uint32_t* __restrict__ prop, uint32_t pcap, uint16_t* __restrict__ tdst,
                    uint32_t* __restrict__ pdst) {
    const uint32_t i = blockIdx.x * (kGatherThreads / 64) + threadIdx.x / 64;
    if (i >= n) return;
    const uint32_t ln = threadIdx.x & 63;
    const uint32_t doc = q[i].doc;
    const int32_t* r = rows + size_t(kRowWords) * i;
    if (tdst) {
        const int64_t o = off[i], len = off[i + 1] - o;
        if (len > 0) {
            const uint16_t* src = text + size_t(doc) * tcap + uint32_t(r[7]);
            for (int64_t k = ln; k < len; k += 64) tdst[o + k] = src[k];
        }
    }
    if (pdst) {
        const int64_t* poff = off + size_t(n) + 1;
        const int64_t o = poff[i], len = poff[i + 1] - o;
        if (len > 0) {
            const uint32_t* src = prop + size_t(doc) * pcap + uint32_t(r[8]);
            for (int64_t k = ln; k < len; k += 64) pdst[o + k] = src[k];
        }
    }
}

// ---- batched reference queries (mtr_get_refs)

// One lane per listed document (docs null: document i): cnt[i] = its references (DocHdr.nrefs; none while the engine
// has no reference table), blk[i] = its 64-reference blocks.  A header that claims more references than the table
// holds, or fewer than none, raises the flag and counts as empty: the host refuses the call before any kernel reads
// the table by it.
constexpr int kCountThreads = 256;
__global__ void __launch_bounds__(kCountThreads)
refs_count_kernel(const DocHdr* __restrict__ hdr, const uint32_t* __restrict__ docs, uint32_t n, int has_table,
                  int refcap, uint64_t* __restrict__ blk, uint64_t* __restrict__ cnt, int32_t* flag) {
    const uint32_t i = blockIdx.x * kCountThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t d = docs ? docs[i] : i;
    int r = has_table ? hdr[d].nrefs : 0;
    if (r < 0 || r > refcap) {
        atomicOr(flag, 1);
        r = 0;
    }
    cnt[i] = uint64_t(r);
    blk[i] = uint64_t((r + 63) / 64);
}

// The work list: one lane per listed document writes its blocks' items (listed index, block) at the document's place in
// the scan of blk (boff, query_scan_kernel's first array).  At most refcap / 64 items a lane.
__global__ void __launch_bounds__(kCountThreads)
refs_work_kernel(const uint64_t* __restrict__ blk, const int64_t* __restrict__ boff, uint32_t n,
                 uint32_t* __restrict__ work) {
    const uint32_t i = blockIdx.x * kCountThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t nb = uint32_t(blk[i]);
    uint32_t* w = work + 2 * size_t(boff[i]);
    for (uint32_t b = 0; b < nb; b++) {
        w[2 * b] = i;
        w[2 * b + 1] = b;
    }
}

// One workgroup (one wave) per work item: references [64 b, 64 b + 64) of listed document i, one round of
// Eng<true>::ref_query, whose words land at the document's place in out (first = the scan of cnt, counted in
// references).  The item is read with scalar loads and made uniform, so the round's cross-lane reads see one document
// and one block in every lane.  Reads document state only; workgroups that share a document do not interfere.
__global__ void __launch_bounds__(NT)
refs_batch_kernel(KParams P, const uint32_t* __restrict__ docs, const uint32_t* __restrict__ work,
                  const int64_t* __restrict__ first, int mode, int info_id, int32_t* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t i = uniu(work[2 * size_t(blockIdx.x)]);
    const int b = uni(int(work[2 * size_t(blockIdx.x) + 1]));
    const uint32_t d = docs ? uniu(docs[i]) : i;
    Eng<true>::ref_query(smem, P, d, out + size_t(mode) * size_t(first[i]), info_id, b, 1);
}

// ---- batched range queries (mtr_get_range_segments)

constexpr int kFirstWords = 4;  // per query: the first round that holds a segment of the range, and what precedes it

// What one lane's leaf gives a range [start, end) of a view, from the leaf's visible length x and its exclusive prefix.
// in: the leaf is a segment of the range.  units: a text segment's units inside the range (clipped at both ends), one
// for a marker when a placeholder is set; tsrc: where they start in the document's text arena.  words: its property
// words (1 + 2 n), pref: where they start in the property arena.  bad: the kBad* bits of a text or a property set that
// does not lie inside its arena (such a leaf counts no units or words; the host refuses the call).  A matrix vector's
// leaves and the parts the caller skipped (want_text / want_props false) give nothing and are not checked.
struct RangeLane {
    bool in;
    int units, words, bad;
    uint32_t tsrc, pref;
};
template <class D>
MTR_DI RangeLane range_lane(const D& L, const KParams& P, uint32_t d, int i, int x, int excl, uint32_t meta, int start,
                            int end, bool matrix, bool want_text, bool place, bool want_props) {
    RangeLane r{};
    r.in = (x > 0) & (excl < end) & (excl + x > start);
    if (!r.in || matrix) return r;
    if (want_text) {
        if (meta & M_MARKER) {
            r.units = place ? 1 : 0;
        } else {
            const int lo = max(start - excl, 0), hi = min(end - excl, x);
            const uint32_t t = L.text[i];
            if (uint64_t(t) + uint64_t(x) <= uint64_t(P.tcap)) {
                r.units = hi - lo;
                r.tsrc = t + uint32_t(lo);
            } else {
                r.bad |= kBadText;
            }
        }
    }
    if (want_props) {
        const uint32_t p = L.props[i];
        if (p != NONE32) {
            const uint64_t ref = p & PN_MASK, pw = uint64_t(P.pcap);
            if (ref >= pw) {
                r.bad |= kBadProps;
            } else {
                const uint64_t words = 1 + 2 * uint64_t(P.prop[size_t(d) * pw + ref]);
                if (ref + words <= pw) {
                    r.words = int(words);
                    r.pref = uint32_t(ref);
                } else {
                    r.bad |= kBadProps;
                }
            }
        }
    }
    return r;
}

// One workgroup (one wave) per query: the segments of [start, end) at the query's view, counted.  The wave walks the
// document's leaves in rounds of 64 with one scan of the visible lengths a round (Eng::view_round: find1's round); a
// leaf is a segment of the range iff it is visible, starts before `end` and ends after `start`.  cnt[i], cnt[n + i],
// cnt[2 n + i] = its segments, its text units and its property words; first[4 i ..] = {the first round that holds
// one (its first slot), the view's length ahead of that round, the live leaves ahead of it (a hole-layout document's
// ordinals)}, where range_write_kernel starts.  The walk ends with the round whose prefix reaches `end`.
// The query is read with scalar loads and made uniform: every loop bound and every cross-lane source lane below is
// the same in all 64 lanes.  parts: kTextHalf | kPropsHalf, the parts to measure and check.
__global__ void __launch_bounds__(NT)
range_count_kernel(KParams P, const mtr_range_query* __restrict__ q, const uint32_t* __restrict__ dkind, int parts,
                   int place, uint64_t* __restrict__ cnt, uint32_t n, int32_t* __restrict__ first, int32_t* flag) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using E = Eng<true>;
    const uint32_t qi = blockIdx.x;
    const uint32_t d = uniu(q[qi].doc);
    const int start = uni(q[qi].start), end = uni(q[qi].end);
    E::D L;
    St s;
    View v;
    E::view_open(L, s, v, smem, P, d, uni(q[qi].ref_seq), uni(q[qi].client));
    const bool matrix = uniu(dkind[d]) != 0;
    const int S = start < end ? s.nseg : 0;
    const bool holes = s.holes != 0;
    int c = 0, live = 0, segs = 0, f_base = -1, f_c = 0, f_live = 0, bad = 0;
    uint64_t units = 0, words = 0;
    for (int base = 0; base < S; base += 64) {
        E::Hot h;
        const int x = E::view_round(L, s, v, base, P.new_length_calc, h);
        const int inc = wave_incl_scan(x);
        const RangeLane r = range_lane(L, P, d, base + lane_id(), x, c + inc - x, h.meta, start, end, matrix,
                                       (parts & kTextHalf) != 0, place != 0, (parts & kPropsHalf) != 0);
        const uint64_t m = __ballot(r.in);
        // (the scans and the ballots run in every round, outside any branch: all 64 lanes take part)
        const int tsum = rdlane(wave_incl_scan(r.units), 63), psum = rdlane(wave_incl_scan(r.words), 63);
        bad |= (__ballot(r.bad & kBadText) ? kBadText : 0) | (__ballot(r.bad & kBadProps) ? kBadProps : 0);
        if (m && f_base < 0) {
            f_base = base;
            f_c = c;
            f_live = live;
        }
        segs += __popcll(m);
        units += uint64_t(uint32_t(tsum));
        words += uint64_t(uint32_t(psum));
        c += rdlane(inc, 63);
        if (holes) live += __popcll(__ballot((base + lane_id() < S) & !(h.meta & M_DEL)));
        if (c >= end) break;
    }
    if (lane_id() == 0) {
        cnt[qi] = uint64_t(segs);
        cnt[size_t(n) + qi] = units;
        cnt[2 * size_t(n) + qi] = words;
        first[kFirstWords * size_t(qi)] = f_base;
        first[kFirstWords * size_t(qi) + 1] = f_c;
        first[kFirstWords * size_t(qi) + 2] = f_live;
        if (bad) atomicOr(flag, bad);
    }
}

// off[0 .. n] = the exclusive scan of the segment counts with its total, then the same of the units and of the words,
// off[3 n + 3] = the flag: query_scan_kernel's scheme for three arrays.
__global__ void __launch_bounds__(kScanThreads)
range_scan_kernel(const uint64_t* __restrict__ cnt, uint32_t n, const int32_t* __restrict__ flag,
                  int64_t* __restrict__ off) {
    __shared__ uint64_t part[3][kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = uint32_t(min(uint64_t(n), uint64_t(t) * chunk)), hi = uint32_t(min(uint64_t(n), uint64_t(lo) + chunk));
    uint64_t own[3] = {0, 0, 0};
    for (uint32_t i = lo; i < hi; i++)
#pragma unroll
        for (int a = 0; a < 3; a++) own[a] += cnt[size_t(a) * n + i];
#pragma unroll
    for (int a = 0; a < 3; a++) part[a][t] = own[a];
    __syncthreads();
    for (uint32_t step = 1; step < kScanThreads; step <<= 1) {
        uint64_t add[3];
#pragma unroll
        for (int a = 0; a < 3; a++) add[a] = t >= step ? part[a][t - step] : 0;
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; a++) part[a][t] += add[a];
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        int64_t* __restrict__ o = off + size_t(a) * (size_t(n) + 1);
        uint64_t run = part[a][t] - own[a];
        for (uint32_t i = lo; i < hi; i++) {
            o[i] = int64_t(run);
            run += cnt[size_t(a) * n + i];
        }
        if (t == kScanThreads - 1) o[n] = int64_t(part[a][t]);
    }
    if (t == kScanThreads - 1) off[3 * size_t(n) + 3] = *flag;
}

// One workgroup (one wave) per query, started at the round range_count_kernel recorded: the same rounds again, this
// time with the places known.  A round's segments are its in-range lanes in lane order (ballot + mbcnt rank); each such
// lane writes its leaf's row (Eng::leaf_row: containing's words for position p_k, which is `start` in the first segment
// and the segment's own start after it) and its text_off / props_off entries from the running carries; then the wave
// copies the clipped units and the property words leaf by leaf, 64 lanes wide (text_kernel's and query_gather_kernel's
// copy).  off = range_scan_kernel's three scans; parts = what range_count_kernel counted by.  rows, toff, tdst, poff,
// pdst: null skips that output.  Every
// length here passed range_count_kernel's bounds checks with the same parts, so every read lies inside the document's
// arenas; the writes end at the totals the host sized the buffers by.
__global__ void __launch_bounds__(NT)
range_write_kernel(KParams P, const mtr_range_query* __restrict__ q, const uint32_t* __restrict__ dkind, int parts,
                   int place, uint32_t n, const int32_t* __restrict__ first, const int64_t* __restrict__ off,
                   int32_t* __restrict__ rows, int64_t* __restrict__ toff, uint16_t* __restrict__ tdst,
                   int64_t* __restrict__ poff, uint32_t* __restrict__ pdst) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using E = Eng<true>;
    const uint32_t qi = blockIdx.x;
    const int64_t* toff_q = off + size_t(n) + 1;
    const int64_t* poff_q = off + 2 * (size_t(n) + 1);
    // (64-bit values made uniform by halves)
    auto uni64 = [](int64_t x) { return int64_t(uint64_t(uniu(uint32_t(x))) | (uint64_t(uniu(uint32_t(uint64_t(x) >> 32))) << 32)); };
    int64_t row = uni64(off[qi]);
    int left = int(uni64(off[qi + 1]) - row);
    if (left <= 0) return;
    int64_t tcar = uni64(toff_q[qi]), pcar = uni64(poff_q[qi]);
    const uint32_t d = uniu(q[qi].doc);
    const int start = uni(q[qi].start), end = uni(q[qi].end);
    E::D L;
    St s;
    View v;
    E::view_open(L, s, v, smem, P, d, uni(q[qi].ref_seq), uni(q[qi].client));
    const bool matrix = uniu(dkind[d]) != 0;
    const int S = s.nseg;
    const bool holes = s.holes != 0;
    int c = uni(first[kFirstWords * size_t(qi) + 1]), live = uni(first[kFirstWords * size_t(qi) + 2]);
    const bool want_text = (parts & kTextHalf) != 0, want_props = (parts & kPropsHalf) != 0;
    const uint16_t* __restrict__ tx = P.text + size_t(d) * size_t(P.tcap);
    const uint32_t* __restrict__ px = P.prop + size_t(d) * size_t(P.pcap);
    for (int base = max(uni(first[kFirstWords * size_t(qi)]), 0); base < S && left > 0; base += 64) {
        const int i = base + lane_id();
        E::Hot h;
        const int x = E::view_round(L, s, v, base, P.new_length_calc, h);
        const int inc = wave_incl_scan(x);
        const int excl = c + inc - x;
        const RangeLane r = range_lane(L, P, d, i, x, excl, h.meta, start, end, matrix, want_text, place != 0, want_props);
        const uint64_t m = __ballot(r.in);
        const uint64_t mlive = holes ? __ballot((i < S) & !(h.meta & M_DEL)) : 0;
        const int tinc = wave_incl_scan(r.units), pinc = wave_incl_scan(r.words);
        if (r.in) {
            const int64_t k = row + __popcll(m & lanes_below());
            if (rows)
                E::leaf_row(L, i, holes ? live + __popcll(mlive & lanes_below()) : i, max(start - excl, 0), excl,
                            rows + size_t(kRowWords) * size_t(k));
            if (toff) toff[k] = tcar + (tinc - r.units);
            if (poff) poff[k] = pcar + (pinc - r.words);
        }
        if (tdst || pdst) {
            const uint32_t marker = h.meta & M_MARKER;
            for (uint64_t mm = m; mm; mm &= mm - 1) {  // (m is a ballot: the same in every lane)
                const int l = uni(first_lane(mm));
                if (tdst) {
                    const int ul = rdlane(r.units, l);
                    const int64_t o = tcar + (rdlane(tinc, l) - ul);
                    const uint32_t src = rdlane(r.tsrc, l);
                    if (rdlane(marker, l)) {
                        if (lane_id() < ul) tdst[o] = uint16_t(place);
                    } else {
                        for (int u = lane_id(); u < ul; u += 64) tdst[o + u] = tx[src + uint32_t(u)];
                    }
                }
                if (pdst) {
                    const int wl = rdlane(r.words, l);
                    const int64_t o = pcar + (rdlane(pinc, l) - wl);
                    const uint32_t src = rdlane(r.pref, l);
                    for (int u = lane_id(); u < wl; u += 64) pdst[o + u] = px[src + uint32_t(u)];
                }
            }
        }
        const int k = __popcll(m);
        row += k;
        left -= k;
        tcar += rdlane(tinc, 63);
        pcar += rdlane(pinc, 63);
        c += rdlane(inc, 63);
        live += __popcll(mlive);
    }
}

// ---- batched position transforms (mtr_transform_positions)

// One workgroup (one wave) per query: a position of the source view (MTR_POS_FROM_VIEW) or a leaf ordinal
// (MTR_POS_FROM_LEAF) mapped into the target view.  Both views are views of the same leaves, so the wave walks them
// once, in rounds of 64, with two view_rounds and two scans a round: the source prefix finds the leaf as find1 does
// (the first lane whose inclusive prefix passes pos; FROM_LEAF: the lane whose ordinal is pos, counted over the live
// slots in a hole-layout document, as range_count_kernel counts them), and the target prefix ahead of that lane is
// where the leaf starts in the target view -- whether or not that view shows it.  The walk leaves in the round that
// finds the leaf; one that finds none ends with both views' lengths, which decides MTR_POS_AT_END.
// The query is read with scalar loads and made uniform: every loop bound and every cross-lane source lane below is the
// same in all 64 lanes, and the scans and ballots of a round run in every lane, outside any branch.
__global__ void __launch_bounds__(NT)
position_kernel(KParams P, const mtr_position_query* __restrict__ q, mtr_position* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using E = Eng<true>;
    const uint32_t qi = blockIdx.x;
    const uint32_t d = uniu(q[qi].doc);
    const int pos = uni(q[qi].pos), off = uni(q[qi].offset);
    const bool by_leaf = uni(q[qi].mode) == MTR_POS_FROM_LEAF;
    E::D L;
    St s;
    View v, t;
    E::view_open(L, s, v, smem, P, d, uni(q[qi].ref_seq), uni(q[qi].client));
    t.ref = uni(q[qi].to_ref_seq);  // (the target view over the same state, as view_open sets up the source)
    t.client = enc_client(uni(q[qi].to_client));
    t.local = (!s.collab || uint32_t(s.local) == t.client) ? 1 : 0;
    const int S = pos < 0 ? 0 : s.nseg;  // (no position and no ordinal is negative: nothing to walk)
    const bool holes = s.holes != 0;
    int cs = 0, ct = 0, live = 0;
    mtr_position r{-1, -1, 0, 0};
    bool found = false;
    for (int base = 0; base < S; base += 64) {
        const int i = base + lane_id();
        E::Hot hs, ht;
        const int xs = E::view_round(L, s, v, base, P.new_length_calc, hs);
        const int xt = E::view_round(L, s, t, base, P.new_length_calc, ht);
        const int incs = wave_incl_scan(xs), inct = wave_incl_scan(xt);
        const bool is_live = (i < S) & !(hs.meta & M_DEL);
        const uint64_t mlive = __ballot(is_live);
        const int li = holes ? live + __popcll(mlive & lanes_below()) : i;  // the lane's ordinal (a live lane's)
        const uint64_t m = __ballot(by_leaf ? (holes ? is_live : i < S) & (li == pos) : (i < S) & (cs + incs > pos));
        if (m) {
            const int l = uni(first_lane(m));
            const int o = by_leaf ? off : pos - (cs + rdlane(incs - xs, l));
            r.pos = ct + rdlane(inct - xt, l) + o;
            r.leaf = rdlane(li, l);
            r.offset = o;
            r.flags = MTR_POS_FOUND | (rdlane(xt, l) > 0 ? MTR_POS_VISIBLE : 0);
            found = true;
            break;
        }
        cs += rdlane(incs, 63);
        ct += rdlane(inct, 63);
        live += __popcll(mlive);
    }
    if (!found && !by_leaf && pos >= 0 && pos == cs) {
        r.pos = ct;
        r.flags = MTR_POS_AT_END;
    }
    if (lane_id() == 0) out[qi] = r;
}

// ---- batched marker search (mtr_find_markers)

constexpr int kHitWords = 6;  // mtr_marker_hit

// Does the property set of leaf i hold a pair (key, v) with v one of vals[0 .. count)?  Per lane: the set [n, k0, v0,
// ...] is read from the document's property arena px after mtr_get_props' two bounds checks (bad = one failed: the leaf
// matches nothing and the host refuses the call); v is looked up in the label's ascending values by binary search.
MTR_DI bool marker_label_match(uint32_t p, const uint32_t* __restrict__ px, uint32_t pcap, uint32_t key,
                               const uint32_t* __restrict__ vals, uint32_t count, bool& bad) {
    if (p == NONE32) return false;
    const uint64_t ref = p & PN_MASK, pw = uint64_t(pcap);
    if (ref >= pw) {
        bad = true;
        return false;
    }
    const uint32_t n = px[ref];
    if (ref + 1 + 2 * uint64_t(n) > pw) {
        bad = true;
        return false;
    }
    bool hit = false;
    for (uint32_t j = 0; j < n && !hit; j++) {
        if (px[ref + 1 + 2 * j] != key) continue;
        const uint32_t v = px[ref + 2 + 2 * j];
        uint32_t lo = 0, hi = count;
        while (lo < hi) {  // the first value >= v
            const uint32_t mid = (lo + hi) >> 1;
            if (vals[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        hit = lo < count && vals[lo] == v;
    }
    return hit;
}

// One workgroup (one wave) per query: one walk of the document's leaves at the query's view, in rounds of 64 with one
// view_round and one scan of the visible lengths a round (range_count_kernel's walk).  A lane's leaf is a candidate
//   PRECEDING / FOLLOWING  when the view shows it (length > 0), its hot fields say marker, it starts at or before
//                          (at or after) pos, and it matches the label.  Only such lanes read their property set,
//                          behind one ballot: a round without visible markers on the wanted side reads none, and
//                          MTR_LABEL_ANY reads none at all.  PRECEDING keeps the highest candidate lane of the last
//                          round that has one and leaves after the round in which the prefix passes pos; FOLLOWING
//                          leaves with the lowest candidate lane of the first round that has one.
//   BY_ID                  when it is the live leaf whose uid the document's ordinal table maps pos to (mk_look on the
//                          remover-head table, as MTR_OP_RELPOS reads it); the walk compares the uids itself rather than
//                          ask find_uid, whose slot hints a query kernel does not carry.  The leaf's start in the view
//                          is the prefix ahead of it whether or not the view shows it (position_kernel's rule).
// The hit's leaf is its tree-order ordinal: the live slots ahead of it in a hole-layout document.  Lane 0 takes
// ref_type, props and seq from leaf_row's words and writes the row.  flag: a property reference outside the arena.
// The query and its label are read with scalar loads and made uniform: every loop bound and every cross-lane source
// lane below is the same in all 64 lanes, and the scans and ballots of a round run in every lane, outside any branch.
__global__ void __launch_bounds__(NT)
marker_find_kernel(KParams P, const mtr_marker_label* __restrict__ labels, const uint32_t* __restrict__ vals,
                   const mtr_marker_query* __restrict__ q, const uint32_t* __restrict__ dkind,
                   int32_t* __restrict__ out, int32_t* flag) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using E = Eng<true>;
    const uint32_t qi = blockIdx.x;
    const uint32_t d = uniu(q[qi].doc);
    const int pos = uni(q[qi].pos), mode = uni(q[qi].mode);
    const bool by_id = mode == MTR_MK_BY_ID, prec = mode == MTR_MK_PRECEDING;
    E::D L;
    St s;
    View v;
    E::view_open(L, s, v, smem, P, d, uni(q[qi].ref_seq), uni(q[qi].client));
    uint32_t key = MTR_LABEL_ANY, count = 0, want = NONE32;
    const uint32_t* __restrict__ lv = vals;
    bool walk = uniu(dkind[d]) == 0;  // (a matrix vector holds no markers and maps no ordinal)
    if (by_id) {
        // (ordinal 2^31 - 1 is never mapped: its table key + 1 wraps to 0, the empty slot's, so it is not looked up)
        const uint64_t mu = (walk && pos >= 0 && pos != INT32_MAX) ? E::mk_look(L.grt(), uint32_t(L.rtmask), uint32_t(pos)) : 0;
        walk = (mu >> 32) != 0;
        want = uint32_t(mu);
    } else {
        const uint32_t li = uniu(q[qi].label);
        key = uniu(labels[li].key);
        count = uniu(labels[li].count);
        lv = vals + uniu(labels[li].first);
    }
    const uint32_t* __restrict__ px = P.prop + size_t(d) * size_t(P.pcap);
    const int S = walk ? s.nseg : 0;
    const bool holes = s.holes != 0;
    int c = 0, live = 0, slot = -1, start = 0, ord = 0, shown = 0, bad = 0;
    for (int base = 0; base < S; base += 64) {
        const int i = base + lane_id();
        E::Hot h;
        const int x = E::view_round(L, s, v, base, P.new_length_calc, h);
        const int inc = wave_incl_scan(x);
        const int excl = c + inc - x;
        const bool is_live = (i < S) & !(h.meta & M_DEL);
        bool cand;
        if (by_id) {
            cand = is_live && L.uid[min(i, S - 1)] == want;
        } else {
            cand = (x > 0) & ((h.meta & M_MARKER) != 0) & (prec ? excl <= pos : excl >= pos);
            if (key != MTR_LABEL_ANY && __ballot(cand)) {  // (uniform: the property path of this round's markers)
                bool b = false;
                if (cand) cand = marker_label_match(L.props[i], px, uint32_t(P.pcap), key, lv, count, b);
                if (__ballot(b)) bad = kBadProps;
            }
        }
        const uint64_t m = __ballot(cand);
        const uint64_t mlive = holes ? __ballot(is_live) : 0;
        if (m) {
            const int l = uni(prec ? last_lane(m) : first_lane(m));
            slot = base + l;
            start = rdlane(excl, l);
            shown = rdlane(x, l);
            ord = holes ? live + __popcll(mlive & ((uint64_t(1) << l) - 1)) : slot;
            if (!prec) break;
        }
        c += rdlane(inc, 63);
        live += __popcll(mlive);
        if (prec && c > pos) break;  // (every later leaf starts past pos)
    }
    if (lane_id() == 0) {
        int32_t* o = out + size_t(kHitWords) * qi;
        if (slot < 0) {
            o[0] = -1; o[1] = -1; o[2] = 0; o[3] = -1; o[4] = 0; o[5] = 0;
        } else {
            int32_t r[kRowWords];
            E::leaf_row(L, slot, ord, 0, start, r);
            o[0] = start;
            o[1] = ord;
            o[2] = r[7];
            o[3] = r[8];
            o[4] = r[3] >= LOCAL_BASE ? -1 : r[3];  // (mtr_segment_info.seq: segment_info_from_row's rule)
            o[5] = MTR_MK_FOUND | (shown > 0 ? MTR_MK_VISIBLE : 0);
        }
        if (bad) atomicOr(flag, bad);
    }
}

// ---- batched interval queries (mtr_query_intervals)

// The device form of a set: mtr_interval_set plus the first of its 32-interval blocks in the work list, which is also
// where its endpoints' key rows start (64 rows a block).
struct IvSet {
    uint32_t doc, first, count, block;
};
constexpr int kIvWorkWords = 8;  // per query: T(start), T(end) as packed keys, the PREVIOUS / NEXT answer, its ties
// The flag word of a call starts as kIvClean; a reference id its document does not have lowers it to the interval's
// index in `refs` (atomicMin: the first one), a header that claims more references than the table holds to
// kIvBadHeader | set.
constexpr uint32_t kIvClean = 0xffffffffu, kIvBadHeader = 0x80000000u;

// A compare key as one word that orders as intervals._ref_key's tuple does: 0 for (0, 0, 0), else (slot + 1, offset).
MTR_DI uint64_t iv_pack(int key, int off) {
    return key < 0 ? 0 : ((uint64_t(uint32_t(key)) + 1) << 32) | uint32_t(off);
}
MTR_DI uint64_t iv_uni64(uint64_t x) {  // (a 64-bit value made uniform by halves)
    return uint64_t(uniu(uint32_t(x))) | (uint64_t(uniu(uint32_t(x >> 32))) << 32);
}
// The largest x of the wave, in every lane (a butterfly of six steps; every lane takes part).
MTR_DI uint64_t iv_wave_max(uint64_t x) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(x)), w, 64));
        const uint32_t hi = uint32_t(__shfl_xor(int(uint32_t(x >> 32)), w, 64));
        const uint64_t y = uint64_t(lo) | (uint64_t(hi) << 32);
        x = y > x ? y : x;
    }
    return x;
}

// One workgroup (one wave) per work item (set, block): the 64 endpoints of intervals [32 b, 32 b + 32) of the set, one
// per lane (lane 2 j the start reference of interval 32 b + j, lane 2 j + 1 its end), looked for in the document's
// leaves as Eng<true>::ref_query's info_id == -3 round looks for a block of the reference table -- the same walk, the
// same words -- but for the named references alone: rows[64 * (set.block + b) + lane] = {position, key (-1: no segment,
// -2: a segment zamboni took out of the tree), offset, 0}.  The work item and the set are read with scalar loads and
// made uniform; the leaf walk's bounds and its cross-lane source lanes are the same in all 64 lanes.
__global__ void __launch_bounds__(NT)
interval_keys_kernel(KParams P, const IvSet* __restrict__ sets, const uint32_t* __restrict__ refs,
                     const uint32_t* __restrict__ work, int4* __restrict__ rows, uint32_t* flag) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using E = Eng<true>;
    const uint32_t si = uniu(work[2 * size_t(blockIdx.x)]), b = uniu(work[2 * size_t(blockIdx.x) + 1]);
    const uint32_t d = uniu(sets[si].doc), first = uniu(sets[si].first), count = uniu(sets[si].count);
    const uint32_t blk = uniu(sets[si].block);
    E::D L;
    St s;
    View v;
    E::view_open(L, s, v, smem, P, d, 0, 0);  // (the state alone: this walk is ref_query's, which takes no view)
    int n = E::rf_uid(L) ? E::nrefs(L) : 0;
    const bool bad_header = n < 0 || n > P.refcap;
    if (bad_header) n = 0;
    const int S = s.nseg;
    const uint32_t k = 32 * b + uint32_t(lane_id() >> 1);
    const bool valid = k < count;
    const uint32_t rid = valid ? refs[2 * (size_t(first) + 32 * size_t(b)) + size_t(lane_id())] : 0;
    const bool have = valid & (rid < uint32_t(n));
    if (valid && !have) atomicMin(flag, bad_header ? (kIvBadHeader | si) : first + k);
    uint32_t u = NONE32, o = 0, t = 0;
    if (have) {
        u = E::rf_uid(L)[rid];
        o = E::rf_off(L)[rid];
        t = E::rf_ty(L)[rid];
    }
    const bool live = have & (u != NONE32) & ((t & (E::RF_HELD | E::RT_TRANSIENT)) != 0);
    const bool want = have & (u != NONE32);
    int res = MTR_DETACHED_POSITION, key = -1;
    bool found = false;
    int carry = 0;
    for (int base = 0; base < S && __ballot(want & !found); base += 64) {
        const int i = base + lane_id();
        const int ic = min(i, S - 1);
        const uint32_t m = L.meta[ic];
        const int rs = L.rseq[ic];
        const bool leaf = (i < S) & !(m & M_DEL);
        const int x = (leaf & (rs == RNONE)) ? L.len[ic] : 0;  // local view: removed leaves count 0
        const int inc = wave_incl_scan(x);
        const int excl = carry + inc - x;
        const uint32_t ui = leaf ? L.uid[ic] : NONE32;
        const int rm = rs != RNONE ? 1 : 0;
        for (int l = 0; l < 64; l++) {  // every endpoint lane looks for its leaf in this round
            const uint32_t ul = rdlane(ui, l);
            const int el = rdlane(excl, l), rl = rdlane(rm, l);
            const bool hit = want & !found & (ul == u);
            res = (hit & live) ? (rl ? 0 : int(o)) + el : res;
            key = hit ? base + l : key;
            found = found | hit;
        }
        carry += rdlane(inc, 63);
    }
    rows[64 * (size_t(blk) + b) + size_t(lane_id())] =
        make_int4(res, (!have || u == NONE32) ? -1 : (found ? key : -2), int(o), 0);
}

// What one lane's interval gives a query, from its two key rows.
struct IvLane {
    uint64_t ks, ke;  // the packed keys of its start and end references
    bool unlinked;    // one of them sits on a segment that left the tree
};
MTR_DI IvLane iv_lane(const int4& a, const int4& b) {
    return IvLane{iv_pack(a.y, a.z), iv_pack(b.y, b.z), a.y == -2 || b.y == -2};
}
// PREVIOUS and NEXT as one maximum: a candidate's end key + 1 (PREVIOUS: the greatest end key at or below T) or its
// complement (NEXT: the least at or above T); 0 = no candidate.  An end key is below 2^63, so neither form is 0.
MTR_DI uint64_t iv_rank(bool prev, bool valid, uint64_t ke, uint64_t t) {
    return !valid ? 0 : prev ? (ke <= t ? ke + 1 : 0) : (ke >= t ? ~ke : 0);
}

// One workgroup (one wave) per query.  T(start) and T(end), the keys two Transient references at those positions of the
// document's local view would have (ref_create's MTR_REF_LOCALVIEW view: find1's leaf as a slot index, and the units
// ahead of the position inside it), come from one walk of the leaves in rounds of 64 with one scan and two ballots a
// round; the walk leaves in the round that settles both.  A position below 0 or at or past the view's length has no
// segment: key 0.  Then the set's intervals, 64 a round, one per lane, from their key rows: OVERLAP counts K(start ref)
// <= T(end) and K(end ref) >= T(start) with a ballot; PREVIOUS / NEXT keep the best end key so far, the smallest k that
// has it and how many have it.  cnt[qi] = the hits, st[qi] = the status (MTR_IVQ_UNLINKED: an endpoint of the set sits
// on a segment that left the tree; no hits then), w[8 qi ..] = {T(start), T(end), k, ties}.
// The query and its set are read with scalar loads and made uniform: every loop bound and every cross-lane source lane
// below is the same in all 64 lanes, and the scans, ballots and reductions of a round run outside any branch.
__global__ void __launch_bounds__(NT)
interval_count_kernel(KParams P, const IvSet* __restrict__ sets, const mtr_interval_query* __restrict__ q,
                      const int4* __restrict__ rows, uint64_t* __restrict__ cnt, uint64_t* __restrict__ st,
                      int32_t* __restrict__ w) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using E = Eng<true>;
    const uint32_t qi = blockIdx.x;
    const uint32_t si = uniu(q[qi].set);
    const int mode = uni(q[qi].mode);
    const int start = uni(q[qi].start), end = mode == MTR_IVQ_OVERLAP ? uni(q[qi].end) : start;
    const uint32_t d = uniu(sets[si].doc), count = uniu(sets[si].count);
    const int4* __restrict__ kr = rows + 64 * size_t(uniu(sets[si].block));
    E::D L;
    St s;
    View v;
    E::view_open(L, s, v, smem, P, d, 0, 0);
    v.ref = s.curseq;  // (the view MTR_REF_LOCALVIEW names, as ref_create sets it up)
    v.client = s.collab ? uint32_t(s.local) : CL_LOCAL;
    v.local = 1;
    uint64_t ts = 0, te = 0;
    bool open_s = start >= 0, open_e = end >= 0;
    const int S = (count > 0 && end >= start) ? s.nseg : 0;  // (no interval, no range: no key is compared)
    int c = 0;
    for (int base = 0; base < S && (open_s || open_e); base += 64) {
        const int i = base + lane_id();
        E::Hot h;
        const int x = E::view_round(L, s, v, base, P.new_length_calc, h);
        const int inc = wave_incl_scan(x);
        const uint64_t ms = __ballot((i < S) & (c + inc > start)), me = __ballot((i < S) & (c + inc > end));
        if (open_s && ms) {
            const int l = uni(first_lane(ms));
            ts = iv_pack(base + l, start - (c + rdlane(inc - x, l)));
            open_s = false;
        }
        if (open_e && me) {
            const int l = uni(first_lane(me));
            te = iv_pack(base + l, end - (c + rdlane(inc - x, l)));
            open_e = false;
        }
        c += rdlane(inc, 63);
    }
    const bool prev = mode == MTR_IVQ_PREVIOUS;
    const bool scan = end >= start;
    int hits = 0, bestk = -1, ties = 0;
    uint64_t best = 0;
    bool unlinked = false;
    for (uint32_t kb = 0; kb < count; kb += 64) {
        const uint32_t k = kb + uint32_t(lane_id());
        const bool valid = k < count;
        const uint32_t kc = valid ? k : count - 1;
        const IvLane x = iv_lane(kr[2 * size_t(kc)], kr[2 * size_t(kc) + 1]);
        unlinked = unlinked | (__ballot(valid & x.unlinked) != 0);
        if (mode == MTR_IVQ_OVERLAP) {
            hits += __popcll(__ballot(valid & scan & (x.ks <= te) & (x.ke >= ts)));
        } else {
            const uint64_t r = iv_rank(prev, valid, x.ke, ts);
            const uint64_t top = iv_uni64(iv_wave_max(r));
            const uint64_t eq = __ballot((r == top) & (top != 0));
            if (top > best) {
                best = top;
                bestk = int(kb) + first_lane(eq);
                ties = __popcll(eq);
            } else if (top == best && top != 0) {
                ties += __popcll(eq);
            }
        }
    }
    if (mode != MTR_IVQ_OVERLAP) hits = best != 0 ? 1 : 0;
    if (lane_id() == 0) {
        cnt[qi] = unlinked ? 0 : uint64_t(hits);
        st[qi] = unlinked ? MTR_IVQ_UNLINKED : 0;
        int4* o = reinterpret_cast<int4*>(w + kIvWorkWords * size_t(qi));
        o[0] = make_int4(int(uint32_t(ts)), int(uint32_t(ts >> 32)), int(uint32_t(te)), int(uint32_t(te >> 32)));
        o[1] = make_int4(bestk, ties, 0, 0);
    }
}

// One workgroup (one wave) per query with hits (first = the scan of the counts): OVERLAP redoes the predicate from the
// work row's two T keys, 64 intervals a round, and a hit lane's place is the hits of the rounds before plus those of
// the lanes below it (ballot + mbcnt, the one-bit wave scan); PREVIOUS / NEXT write the one interval the count kernel
// found.  A row is 32 bytes, written as two 16-byte stores.  The place is checked against the query's count, so the
// writes end at the total the host sized the buffer by.
__global__ void __launch_bounds__(NT)
interval_write_kernel(const IvSet* __restrict__ sets, const mtr_interval_query* __restrict__ q,
                      const int4* __restrict__ rows, const int64_t* __restrict__ first, const int32_t* __restrict__ w,
                      int4* __restrict__ out) {
    const uint32_t qi = blockIdx.x;
    const int64_t row = int64_t(iv_uni64(uint64_t(first[qi])));
    const int n = int(int64_t(iv_uni64(uint64_t(first[qi + 1]))) - row);
    if (n <= 0) return;
    const uint32_t si = uniu(q[qi].set);
    const int mode = uni(q[qi].mode);
    const uint32_t count = uniu(sets[si].count);
    const int4* __restrict__ kr = rows + 64 * size_t(uniu(sets[si].block));
    const int4 w0 = reinterpret_cast<const int4*>(w + kIvWorkWords * size_t(qi))[0];
    const int4 w1 = reinterpret_cast<const int4*>(w + kIvWorkWords * size_t(qi))[1];
    const uint64_t ts = iv_uni64(uint64_t(uint32_t(w0.x)) | (uint64_t(uint32_t(w0.y)) << 32));
    const uint64_t te = iv_uni64(uint64_t(uint32_t(w0.z)) | (uint64_t(uint32_t(w0.w)) << 32));
    if (mode != MTR_IVQ_OVERLAP) {
        const int k = uni(w1.x), ties = uni(w1.y);
        if (lane_id() == 0 && k >= 0 && uint32_t(k) < count) {
            const int4 a = kr[2 * size_t(k)], b = kr[2 * size_t(k) + 1];
            out[2 * size_t(row)] = make_int4(k, a.x, b.x, a.y);
            out[2 * size_t(row) + 1] = make_int4(a.z, b.y, b.z, ties > 1 ? MTR_IVQ_TIE : 0);
        }
        return;
    }
    int done = 0;
    for (uint32_t kb = 0; kb < count && done < n; kb += 64) {
        const uint32_t k = kb + uint32_t(lane_id());
        const bool valid = k < count;
        const uint32_t kc = valid ? k : count - 1;
        const int4 a = kr[2 * size_t(kc)], b = kr[2 * size_t(kc) + 1];
        const IvLane x = iv_lane(a, b);
        const bool hit = valid & (x.ks <= te) & (x.ke >= ts);
        const uint64_t m = __ballot(hit);
        const int at = done + __popcll(m & lanes_below());
        if (hit && at < n) {
            out[2 * (size_t(row) + size_t(at))] = make_int4(int(k), a.x, b.x, a.y);
            out[2 * (size_t(row) + size_t(at)) + 1] = make_int4(a.z, b.y, b.z, 0);
        }
        done += __popcll(m);
    }
}

// ---- batched delta records (mtr_get_deltas_batch)

constexpr int kBadHeader = 4;  // (a bit of the device flag) a DocHdr.dused outside the document's slice of the records
constexpr int kDeltaThreads = 256;  // four waves a workgroup, one listed document a wave

MTR_DI int64_t uni_i64(int64_t x) {  // (a 64-bit value made uniform by halves)
    return int64_t(uint64_t(uniu(uint32_t(x))) | (uint64_t(uniu(uint32_t(uint64_t(x) >> 32))) << 32));
}

// The property words one record adds: those mtr_get_props returns for a MTR_DELTA_REGEN_X record's `len` (1 + 2 n),
// none for any other record.  px = the document's property arena; bad = the set does not lie inside it (the two checks
// containing_batch_kernel makes; such a record counts no words and the host refuses the call).
MTR_DI int delta_words(uint32_t kind, int32_t len, const uint32_t* __restrict__ px, uint32_t pcap, bool& bad) {
    if (kind != MTR_DELTA_REGEN_X || len < 0) return 0;
    const uint64_t ref = uint32_t(len), pw = uint64_t(pcap);
    if (ref < pw) {
        const uint64_t words = 1 + 2 * uint64_t(px[ref]);
        if (ref + words <= pw) return int(words);
    }
    bad = true;
    return 0;
}

// One wave per listed document (docs null: document i): cnt[i] = its records (DocHdr.dused) when the last batch held it
// (d < limit: that batch's n_docs, or 0 while it recorded nothing), else none.  A header whose count is negative or
// larger than the document's slice raises kBadHeader and counts as empty: nothing reads the records by it.  With
// want_props, wcnt[i] = the property words of the document's records, which the wave reads 64 a round (kind and len
// alone); a matrix vector's REGEN_X fields are handles and count none.  A document without records leaves at once.
// The listed index, the document and the count are uniform: every scan and ballot below runs in all 64 lanes.
__global__ void __launch_bounds__(kDeltaThreads)
delta_count_kernel(const DocHdr* __restrict__ hdr, const uint32_t* __restrict__ docs, uint32_t n, uint32_t limit,
                   const uint64_t* __restrict__ doff, const mtr_delta* __restrict__ delta,
                   const uint32_t* __restrict__ dkind, const uint32_t* __restrict__ prop, uint32_t pcap, int want_props,
                   uint64_t* __restrict__ wcnt, uint64_t* __restrict__ cnt, int32_t* flag) {
    const uint32_t i = uniu(blockIdx.x * (kDeltaThreads / 64) + threadIdx.x / 64);
    if (i >= n) return;
    const uint32_t d = docs ? uniu(docs[i]) : i;
    int r = 0, bad = 0;
    uint64_t o = 0;
    if (d < limit) {
        r = uni(hdr[d].dused);
        o = uint64_t(uni_i64(int64_t(doff[d])));
        const uint64_t slice = uint64_t(uni_i64(int64_t(doff[d + 1]))) - o;
        if (r < 0 || uint64_t(r) > slice) {
            bad = kBadHeader;
            r = 0;
        }
    }
    uint64_t words = 0;
    if (r > 0 && want_props && uniu(dkind[d]) == 0) {
        const mtr_delta* __restrict__ rec = delta + o;
        const uint32_t* __restrict__ px = prop + size_t(d) * size_t(pcap);
        for (int base = 0; base < r; base += 64) {
            const int k = base + lane_id();
            bool b = false;
            int w = 0;
            if (k < r) w = delta_words(rec[k].kind, rec[k].len, px, pcap, b);
            words += uint64_t(uint32_t(rdlane(wave_incl_scan(w), 63)));
            if (__ballot(b)) bad |= kBadProps;
        }
    }
    if (lane_id() == 0) {
        cnt[i] = uint64_t(r);
        wcnt[i] = words;
        if (bad) atomicOr(flag, bad);
    }
}

// One wave per listed document, 64 records a round: lane k copies record k as one 16-byte unit (the slices start at
// 16 * doff[d] bytes of a hipMalloc'd buffer) to its place in recs, rfirst[i] + k; writes the record's poff entry from
// the round's scan of the word counts and the running carry (wfirst[i] at the start); then the wave copies the
// property sets one after the other, 64 lanes wide (range_write_kernel's copy).  rfirst, wfirst = query_scan_kernel's
// scans of cnt and wcnt.  recs null skips the records; poff and pdst both null skip the words' part (the arena is not
// read); either may be null alone.  Every set here passed delta_count_kernel's checks, so every read lies inside the
// document's arena; the writes end at the totals the host sized the buffers by.
__global__ void __launch_bounds__(kDeltaThreads)
delta_records_kernel(const uint32_t* __restrict__ docs, uint32_t n, const int64_t* __restrict__ rfirst,
                     const int64_t* __restrict__ wfirst, const uint64_t* __restrict__ doff,
                     const uint4* __restrict__ delta, const uint32_t* __restrict__ dkind,
                     const uint32_t* __restrict__ prop, uint32_t pcap, uint4* __restrict__ recs,
                     int64_t* __restrict__ poff, uint32_t* __restrict__ pdst) {
    const uint32_t i = uniu(blockIdx.x * (kDeltaThreads / 64) + threadIdx.x / 64);
    if (i >= n) return;
    const int64_t row = uni_i64(rfirst[i]);
    const int r = int(uni_i64(rfirst[i + 1]) - row);
    if (r <= 0) return;
    const uint32_t d = docs ? uniu(docs[i]) : i;
    const uint4* __restrict__ src = delta + uint64_t(uni_i64(int64_t(doff[d])));
    const uint32_t* __restrict__ px = prop + size_t(d) * size_t(pcap);
    const bool words_part = (poff || pdst) && uniu(dkind[d]) == 0;
    int64_t pcar = uni_i64(wfirst[i]);
    for (int base = 0; base < r; base += 64) {
        const int k = base + lane_id();
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < r) {
            v = src[k];
            if (recs) recs[row + k] = v;
        }
        bool b = false;  // (checked by the count kernel: never set here)
        const int w = (words_part && k < r) ? delta_words(v.w, int32_t(v.z), px, pcap, b) : 0;
        const int winc = wave_incl_scan(w);
        if (poff && k < r) poff[row + k] = pcar + (winc - w);
        const uint64_t m = __ballot(w > 0);
        if (pdst) {
            for (uint64_t mm = m; mm; mm &= mm - 1) {  // (m is a ballot: the same in every lane)
                const int l = uni(first_lane(mm));
                const int wl = rdlane(w, l);
                const int64_t o = pcar + (rdlane(winc, l) - wl);
                const uint32_t s = rdlane(v.z, l);
                for (int u = lane_id(); u < wl; u += 64) pdst[o + u] = px[s + uint32_t(u)];
            }
        }
        pcar += rdlane(winc, 63);
    }
}

}  // namespace

void mtr::query_params(const mtr_engine* e, KParams& P) {
    P = KParams{};
    P.hdr = e->hdr.p;
    P.seg = e->seg.p;
    P.heap = e->heap.p;
    P.text = e->text.p;
    P.prop = e->prop.p;
    P.rm = e->rm.p;
    P.segcap = int(e->caps.max_segments);
    P.hcap = int(e->caps.heap_entries);
    P.tcap = int(e->caps.text_units);
    P.pcap = int(e->caps.prop_words);
    P.rcap = int(e->caps.remover_cells);
    P.rtab = e->rtab;
    P.new_length_calc = e->opt.new_length_calc;
    P.n_docs = e->n_docs;
}

void mtr::segment_info_from_row(const int32_t* r, int32_t pos, mtr_segment_info* info) {
    std::memset(info, 0, sizeof(*info));
    info->leaf = r[0];
    if (r[0] < 0) {
        info->start = pos >= 0 ? r[9] : 0;  // the view's length (getLength at that view) when pos is past its end
        return;
    }
    info->offset = r[1];
    info->length = r[2];
    // pending local values are kept above every sequence number (LOCAL_BASE + localSeq, apply.hip.h):
    // report them as the reference holds them, UnassignedSequenceNumber plus the localSeq
    info->seq = r[3] >= LOCAL_BASE ? -1 : r[3];
    info->local_seq = r[3] >= LOCAL_BASE ? r[3] - LOCAL_BASE : -1;
    info->client = r[4];
    info->removed = r[5] != -1;
    info->removed_seq = r[5] >= LOCAL_BASE ? -1 : r[5];
    info->local_removed_seq = r[5] >= LOCAL_BASE ? r[5] - LOCAL_BASE : -1;
    info->marker = r[6];
    info->ref_type = r[7];
    info->props = r[8];
    info->start = r[9];
    info->groups = r[10];
}

extern "C" int64_t mtr_get_containing_segments(mtr_engine* e, const mtr_view_query* q, uint32_t n,
                                               mtr_segment_info* info, uint16_t* text, int64_t text_cap,
                                               int64_t* text_off, uint32_t* props, int64_t props_cap,
                                               int64_t* props_off) {
    HIPCHK(hipSetDevice(e->device));
    if (n && (!q || !info)) {
        set_err("mtr_get_containing_segments: queries and info are required");
        return -1;
    }
    for (uint32_t i = 0; i < n; i++)
        if (q[i].doc >= e->max_docs) {
            set_err("mtr_get_containing_segments: bad document " + std::to_string(q[i].doc) + " in query " +
                    std::to_string(i));
            return -1;
        }
    if (n == 0) {
        if (text_off) text_off[0] = 0;
        if (props_off) props_off[0] = 0;
        return 0;
    }
    mtr_engine::SegmentQueries& w = e->squery;
    const size_t N = n, noff = 2 * N + 3;
    if (w.q.ensure(N) || w.rows.ensure(N * kRowWords) || w.len.ensure(2 * N) || w.off.ensure(noff) || w.flag.ensure(1))
        return -1;
    KParams P;
    query_params(e, P);
    const int halves = (text_off ? kTextHalf : 0) | (props_off ? kPropsHalf : 0);
    HIPCHK(hipMemcpyAsync(w.q.p, q, N * sizeof(mtr_view_query), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(w.flag.p, 0, sizeof(int32_t), e->stream));
    containing_batch_kernel<<<n, NT, lds_bytes_global_mode(int(P.segcap)), e->stream>>>(
        P, w.q.p, e->dkind.p, halves, w.rows.p, w.len.p, w.len.p + N, w.flag.p);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> rows(N * kRowWords);
    std::vector<int64_t> off(noff, 0);
    HIPCHK(hipMemcpyAsync(rows.data(), w.rows.p, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (halves) {  // (both halves skipped: the rows are the whole answer)
        query_scan_kernel<<<1, kScanThreads, 0, e->stream>>>(w.len.p, w.len.p + N, n, w.flag.p, w.off.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(off.data(), w.off.p, noff * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    if (off[2 * N + 2]) {
        set_err(off[2 * N + 2] & kBadProps ? "mtr_get_containing_segments: reference outside the property arena"
                                           : "mtr_get_containing_segments: segment text outside the text arena");
        return -1;
    }
    for (uint32_t i = 0; i < n; i++) segment_info_from_row(rows.data() + size_t(kRowWords) * i, q[i].pos, &info[i]);
    const int64_t* toff = off.data();
    const int64_t* poff = off.data() + N + 1;
    if (text_off) std::memcpy(text_off, toff, (N + 1) * sizeof(int64_t));
    if (props_off) std::memcpy(props_off, poff, (N + 1) * sizeof(int64_t));
    const bool want_text = text_off && text, want_props = props_off && props;
    if ((want_text && toff[N] > text_cap) || (want_props && poff[N] > props_cap)) return MTR_SUMMARY_TOO_SMALL;
    const bool get_text = want_text && toff[N] > 0, get_props = want_props && poff[N] > 0;
    if (!get_text && !get_props) return n;
    if ((get_text && w.text.ensure(size_t(toff[N]))) || (get_props && w.props.ensure(size_t(poff[N])))) return -1;
    const uint32_t per = kGatherThreads / 64;
    query_gather_kernel<<<(n + per - 1) / per, kGatherThreads, 0, e->stream>>>(
        w.q.p, w.rows.p, w.off.p, n, e->text.p, e->caps.text_units, e->prop.p, e->caps.prop_words,
        get_text ? w.text.p : nullptr, get_props ? w.props.p : nullptr);
    HIPCHK(hipGetLastError());
    if (get_text)
        HIPCHK(hipMemcpyAsync(text, w.text.p, size_t(toff[N]) * sizeof(uint16_t), hipMemcpyDeviceToHost, e->stream));
    if (get_props)
        HIPCHK(hipMemcpyAsync(props, w.props.p, size_t(poff[N]) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return n;
}

extern "C" int64_t mtr_get_refs(mtr_engine* e, const uint32_t* docs, uint32_t n, int32_t mode, int32_t* out,
                                int64_t cap_words, int64_t* doc_first) {
    HIPCHK(hipSetDevice(e->device));
    if (mode != MTR_REFS_POSITIONS && mode != MTR_REFS_STATES && mode != MTR_REFS_KEYS) {
        set_err("mtr_get_refs: bad mode " + std::to_string(mode) + " (the words per reference: 1, 2 or 4)");
        return -1;
    }
    if (n && !doc_first) {
        set_err("mtr_get_refs: doc_first is required");
        return -1;
    }
    for (uint32_t i = 0; i < n; i++)  // (a null list names documents 0 .. n - 1: the first bad one is max_docs)
        if ((docs ? docs[i] : i) >= e->max_docs) {
            set_err("mtr_get_refs: bad document " + std::to_string(docs ? docs[i] : i) + " at index " + std::to_string(i));
            return -1;
        }
    if (n == 0) {
        if (doc_first) doc_first[0] = 0;
        return 0;
    }
    mtr_engine::RefQueries& w = e->rquery;
    const size_t N = n, noff = 2 * N + 3;
    if ((docs && w.list.ensure(N)) || w.len.ensure(2 * N) || w.off.ensure(noff) || w.flag.ensure(1)) return -1;
    if (docs) HIPCHK(hipMemcpyAsync(w.list.p, docs, N * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    const uint32_t* list = docs ? w.list.p : nullptr;
    HIPCHK(hipMemsetAsync(w.flag.p, 0, sizeof(int32_t), e->stream));
    // len = [blocks | references], so that off = [block offsets (n + 1) | doc_first (n + 1) | flag] and the read-back
    // is one run: the block total, doc_first, the flag
    uint64_t* blk = w.len.p;
    uint64_t* cnt = w.len.p + N;
    const uint32_t grid = uint32_t((N + kCountThreads - 1) / kCountThreads);
    refs_count_kernel<<<grid, kCountThreads, 0, e->stream>>>(e->hdr.p, list, n, e->refs.p != nullptr,
                                                            int(e->caps.ref_slots), blk, cnt, w.flag.p);
    HIPCHK(hipGetLastError());
    query_scan_kernel<<<1, kScanThreads, 0, e->stream>>>(blk, cnt, n, w.flag.p, w.off.p);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> h(N + 3);  // off[n .. 2 n + 2]
    HIPCHK(hipMemcpyAsync(h.data(), w.off.p + N, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (h[N + 2]) {
        set_err("mtr_get_refs: a document's header holds more references than caps.ref_slots");
        return -1;
    }
    const int64_t blocks = h[0], total = h[N + 1];
    std::memcpy(doc_first, h.data() + 1, (N + 1) * sizeof(int64_t));
    if (!out) return total;
    if (cap_words < int64_t(mode) * total) return MTR_SUMMARY_TOO_SMALL;
    if (total == 0) return 0;
    if (blocks > int64_t(INT32_MAX)) {
        set_err("mtr_get_refs: too many reference blocks for one launch: " + std::to_string(blocks));
        return -1;
    }
    const size_t words = size_t(mode) * size_t(total);
    if (w.work.ensure(2 * size_t(blocks)) || w.words.ensure(words)) return -1;
    refs_work_kernel<<<grid, kCountThreads, 0, e->stream>>>(blk, w.off.p, n, w.work.p);
    HIPCHK(hipGetLastError());
    KParams P;
    query_params(e, P);
    P.refs = e->refs.p;
    P.refcap = int(e->caps.ref_slots);
    const int info_id = mode == MTR_REFS_POSITIONS ? -1 : mode == MTR_REFS_STATES ? -2 : -3;
    refs_batch_kernel<<<uint32_t(blocks), NT, lds_bytes_global_mode(int(P.segcap)), e->stream>>>(
        P, list, w.work.p, w.off.p + N + 1, mode, info_id, w.words.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, w.words.p, words * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return total;
}

extern "C" int64_t mtr_get_range_segments(mtr_engine* e, const mtr_range_query* q, uint32_t n, uint16_t placeholder,
                                          int64_t* seg_first, mtr_segment_info* info, int64_t info_cap, uint16_t* text,
                                          int64_t text_cap, int64_t* text_first, int64_t* text_off, uint32_t* props,
                                          int64_t props_cap, int64_t* props_off) {
    HIPCHK(hipSetDevice(e->device));
    if (n && (!q || !seg_first)) {
        set_err("mtr_get_range_segments: queries and seg_first are required");
        return -1;
    }
    for (uint32_t i = 0; i < n; i++) {
        const char* what = q[i].doc >= e->max_docs ? "bad document" : q[i].start < 0 ? "start < 0"
                           : q[i].end < q[i].start ? "end < start" : nullptr;
        if (what) {
            set_err("mtr_get_range_segments: " + std::string(what) + " in query " + std::to_string(i) + " (document " +
                    std::to_string(q[i].doc) + ", [" + std::to_string(q[i].start) + ", " + std::to_string(q[i].end) + "))");
            return -1;
        }
    }
    if (n == 0) {
        for (int64_t* o : {seg_first, text_first, text_off, props_off})
            if (o) o[0] = 0;
        return 0;
    }
    const bool text_part = text_first || text_off, props_part = props_off != nullptr;
    const int parts = (text_part ? kTextHalf : 0) | (props_part ? kPropsHalf : 0);
    mtr_engine::RangeQueries& w = e->range;
    const size_t N = n, noff = 3 * N + 4;
    if (w.q.ensure(N) || w.cnt.ensure(3 * N) || w.first.ensure(kFirstWords * N) || w.off.ensure(noff) || w.flag.ensure(1))
        return -1;
    KParams P;
    query_params(e, P);
    const size_t lds = lds_bytes_global_mode(int(P.segcap));
    HIPCHK(hipMemcpyAsync(w.q.p, q, N * sizeof(mtr_range_query), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(w.flag.p, 0, sizeof(int32_t), e->stream));
    range_count_kernel<<<n, NT, lds, e->stream>>>(P, w.q.p, e->dkind.p, parts, int(placeholder), w.cnt.p, n, w.first.p,
                                                  w.flag.p);
    HIPCHK(hipGetLastError());
    range_scan_kernel<<<1, kScanThreads, 0, e->stream>>>(w.cnt.p, n, w.flag.p, w.off.p);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> off(noff);
    HIPCHK(hipMemcpyAsync(off.data(), w.off.p, noff * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (off[noff - 1]) {
        set_err(off[noff - 1] & kBadProps ? "mtr_get_range_segments: reference outside the property arena"
                                          : "mtr_get_range_segments: segment text outside the text arena");
        return -1;
    }
    const int64_t* sfirst = off.data();
    const int64_t* tfirst = off.data() + N + 1;
    const int64_t total = sfirst[N], units = tfirst[N], words = off[3 * N + 2];
    std::memcpy(seg_first, sfirst, (N + 1) * sizeof(int64_t));
    if (text_first) std::memcpy(text_first, tfirst, (N + 1) * sizeof(int64_t));
    const bool too_small = (info && info_cap < total) || (text_part && text && text_cap < units) ||
                           (props_part && props && props_cap < words);
    const bool get_rows = info && !too_small && total > 0;
    const bool get_text = text_part && text && !too_small && units > 0;
    const bool get_props = props_part && props && !too_small && words > 0;
    const bool get_toff = text_off && total > 0, get_poff = props_off && total > 0;
    if (text_off) text_off[total] = units;
    if (props_off) props_off[total] = words;
    if (get_rows || get_text || get_props || get_toff || get_poff) {
        const size_t T = size_t(total);
        if ((get_rows && w.rows.ensure(T * kRowWords)) || (get_toff && w.toff.ensure(T)) || (get_poff && w.poff.ensure(T)) ||
            (get_text && w.text.ensure(size_t(units))) || (get_props && w.props.ensure(size_t(words))))
            return -1;
        // (the parts as counted: a part the caller asked for keeps its carries and clips, whichever of its outputs go)
        range_write_kernel<<<n, NT, lds, e->stream>>>(
            P, w.q.p, e->dkind.p, parts, int(placeholder), n, w.first.p, w.off.p, get_rows ? w.rows.p : nullptr,
            get_toff ? w.toff.p : nullptr, get_text ? w.text.p : nullptr, get_poff ? w.poff.p : nullptr,
            get_props ? w.props.p : nullptr);
        HIPCHK(hipGetLastError());
        std::vector<int32_t> rows(get_rows ? T * kRowWords : 0);
        if (get_rows)
            HIPCHK(hipMemcpyAsync(rows.data(), w.rows.p, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        if (get_toff) HIPCHK(hipMemcpyAsync(text_off, w.toff.p, T * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
        if (get_poff) HIPCHK(hipMemcpyAsync(props_off, w.poff.p, T * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
        if (get_text)
            HIPCHK(hipMemcpyAsync(text, w.text.p, size_t(units) * sizeof(uint16_t), hipMemcpyDeviceToHost, e->stream));
        if (get_props)
            HIPCHK(hipMemcpyAsync(props, w.props.p, size_t(words) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (get_rows)
            for (uint32_t i = 0; i < n; i++)
                for (int64_t k = sfirst[i]; k < sfirst[i + 1]; k++)
                    segment_info_from_row(rows.data() + size_t(kRowWords) * size_t(k), q[i].start, &info[k]);
    }
    return too_small ? MTR_SUMMARY_TOO_SMALL : total;
}

extern "C" int64_t mtr_transform_positions(mtr_engine* e, const mtr_position_query* q, uint32_t n, mtr_position* out) {
    HIPCHK(hipSetDevice(e->device));
    if (n && (!q || !out)) {
        set_err("mtr_transform_positions: queries and out are required");
        return -1;
    }
    for (uint32_t i = 0; i < n; i++) {
        const bool mode_ok = q[i].mode == MTR_POS_FROM_VIEW || q[i].mode == MTR_POS_FROM_LEAF;
        const char* what = q[i].doc >= e->max_docs ? "bad document" : !mode_ok ? "bad mode" : q[i].offset < 0 ? "offset < 0"
                           : (q[i].mode == MTR_POS_FROM_VIEW && q[i].offset != 0) ? "an offset in MTR_POS_FROM_VIEW mode"
                           : nullptr;
        if (what) {
            set_err("mtr_transform_positions: " + std::string(what) + " in query " + std::to_string(i) + " (document " +
                    std::to_string(q[i].doc) + ", mode " + std::to_string(q[i].mode) + ", offset " +
                    std::to_string(q[i].offset) + ")");
            return -1;
        }
    }
    if (n == 0) return 0;
    mtr_engine::SegmentQueries& w = e->squery;
    const size_t N = n;
    if (w.pq.ensure(N) || w.pos.ensure(N)) return -1;
    KParams P;
    query_params(e, P);
    HIPCHK(hipMemcpyAsync(w.pq.p, q, N * sizeof(mtr_position_query), hipMemcpyHostToDevice, e->stream));
    position_kernel<<<n, NT, lds_bytes_global_mode(int(P.segcap)), e->stream>>>(P, w.pq.p, w.pos.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, w.pos.p, N * sizeof(mtr_position), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return n;
}

extern "C" int64_t mtr_query_intervals(mtr_engine* e, const mtr_interval_set* sets, uint32_t n_sets, const uint32_t* refs,
                                       uint32_t n_intervals, const mtr_interval_query* q, uint32_t n, int64_t* hit_first,
                                       int32_t* status, mtr_interval_hit* hits, int64_t hit_cap) {
    HIPCHK(hipSetDevice(e->device));
    const std::string name = "mtr_query_intervals: ";
    if (n && (!q || !hit_first || !status || (n_sets && !sets) || (n_intervals && !refs))) {
        set_err(name + "sets, refs, queries, hit_first and status are required");
        return -1;
    }
    if (n_intervals >= kIvBadHeader || n_sets >= kIvBadHeader) {  // (the flag word carries either index in 31 bits)
        set_err(name + "too many intervals or sets: " + std::to_string(n_intervals) + ", " + std::to_string(n_sets));
        return -1;
    }
    uint64_t blocks = 0;
    for (uint32_t i = 0; sets && i < n_sets; i++) {
        const char* what = sets[i].doc >= e->max_docs ? "bad document"
                           : uint64_t(sets[i].first) + sets[i].count > n_intervals ? "intervals past n_intervals" : nullptr;
        if (what) {
            set_err(name + what + " in set " + std::to_string(i) + " (document " + std::to_string(sets[i].doc) +
                    ", intervals [" + std::to_string(sets[i].first) + ", +" + std::to_string(sets[i].count) + "))");
            return -1;
        }
        blocks += (uint64_t(sets[i].count) + 31) / 32;
    }
    for (uint32_t i = 0; i < n; i++) {
        const bool mode_ok = q[i].mode == MTR_IVQ_OVERLAP || q[i].mode == MTR_IVQ_PREVIOUS || q[i].mode == MTR_IVQ_NEXT;
        const char* what = q[i].set >= n_sets ? "bad set" : !mode_ok ? "bad mode" : nullptr;
        if (what) {
            set_err(name + what + " in query " + std::to_string(i) + " (set " + std::to_string(q[i].set) + ", mode " +
                    std::to_string(q[i].mode) + ")");
            return -1;
        }
    }
    if (n == 0) {
        if (hit_first) hit_first[0] = 0;
        return 0;
    }
    if (blocks > uint64_t(INT32_MAX)) {
        set_err(name + "too many interval blocks for one launch: " + std::to_string(blocks));
        return -1;
    }
    // one upload: the sets in their device form, the queries, the work list of the keys kernel, the reference ids
    const size_t N = n, NS = n_sets, NB = size_t(blocks), NI = n_intervals, noff = 2 * N + 3;
    const size_t set_at = 0, q_at = set_at + 4 * NS, work_at = q_at + 4 * N, refs_at = work_at + 2 * NB;
    std::vector<uint32_t> up(refs_at + 2 * NI);
    uint32_t block = 0;
    for (uint32_t i = 0; i < n_sets; i++) {
        const uint32_t nb = uint32_t((uint64_t(sets[i].count) + 31) / 32);
        const uint32_t rec[4] = {sets[i].doc, sets[i].first, sets[i].count, block};
        std::memcpy(&up[set_at + 4 * size_t(i)], rec, sizeof(rec));
        for (uint32_t b = 0; b < nb; b++) {
            up[work_at + 2 * (size_t(block) + b)] = i;
            up[work_at + 2 * (size_t(block) + b) + 1] = b;
        }
        block += nb;
    }
    static_assert(sizeof(mtr_interval_set) == 12 && sizeof(mtr_interval_query) == 16 && sizeof(mtr_interval_hit) == 32 &&
                      sizeof(IvSet) == 16,
                  "layout");
    std::memcpy(&up[q_at], q, N * sizeof(mtr_interval_query));
    if (NI) std::memcpy(&up[refs_at], refs, 2 * NI * sizeof(uint32_t));
    mtr_engine::IntervalQueries& w = e->ivquery;
    if (w.up.ensure(up.size()) || w.keys.ensure(4 * 64 * std::max<size_t>(NB, 1)) || w.len.ensure(2 * N) ||
        w.off.ensure(noff) || w.flag.ensure(1) || w.work.ensure(kIvWorkWords * N))
        return -1;
    KParams P;
    query_params(e, P);
    P.refs = e->refs.p;
    P.refcap = int(e->caps.ref_slots);
    const size_t lds = lds_bytes_global_mode(int(P.segcap));
    const IvSet* dsets = reinterpret_cast<const IvSet*>(w.up.p + set_at);
    const mtr_interval_query* dq = reinterpret_cast<const mtr_interval_query*>(w.up.p + q_at);
    int4* keys = reinterpret_cast<int4*>(w.keys.p);
    HIPCHK(hipMemcpyAsync(w.up.p, up.data(), up.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(w.flag.p, 0xff, sizeof(int32_t), e->stream));  // kIvClean
    if (NB) {
        interval_keys_kernel<<<uint32_t(NB), NT, lds, e->stream>>>(P, dsets, w.up.p + refs_at, w.up.p + work_at, keys,
                                                                   reinterpret_cast<uint32_t*>(w.flag.p));
        HIPCHK(hipGetLastError());
    }
    // len = [hits | status], so that off = [hit_first (n + 1) | the scan of the status words (n + 1) | flag]: one copy
    interval_count_kernel<<<n, NT, lds, e->stream>>>(P, dsets, dq, keys, w.len.p, w.len.p + N, w.work.p);
    HIPCHK(hipGetLastError());
    query_scan_kernel<<<1, kScanThreads, 0, e->stream>>>(w.len.p, w.len.p + N, n, w.flag.p, w.off.p);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> off(noff);
    HIPCHK(hipMemcpyAsync(off.data(), w.off.p, noff * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const uint32_t f = uint32_t(off[2 * N + 2]);
    if (f != kIvClean) {
        if (f & kIvBadHeader) {
            set_err(name + "the header of set " + std::to_string(f & ~kIvBadHeader) +
                    "'s document holds more references than caps.ref_slots");
            return -1;
        }
        uint32_t si = 0;  // (the first set that holds interval f of `refs`)
        while (si < n_sets && !(f >= sets[si].first && f - sets[si].first < sets[si].count)) si++;
        set_err(name + "a reference id the document does not have in set " + std::to_string(si) + ", interval " +
                std::to_string(si < n_sets ? f - sets[si].first : f));
        return -1;
    }
    const int64_t total = off[N];
    std::memcpy(hit_first, off.data(), (N + 1) * sizeof(int64_t));
    for (size_t i = 0; i < N; i++) status[i] = int32_t(off[N + 2 + i] - off[N + 1 + i]);
    if (!hits) return total;
    if (hit_cap < total) return MTR_SUMMARY_TOO_SMALL;
    if (total == 0) return 0;
    if (w.hits.ensure(size_t(total))) return -1;
    interval_write_kernel<<<n, NT, 0, e->stream>>>(dsets, dq, keys, w.off.p, w.work.p, reinterpret_cast<int4*>(w.hits.p));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hits, w.hits.p, size_t(total) * sizeof(mtr_interval_hit), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return total;
}

extern "C" int64_t mtr_find_markers(mtr_engine* e, const mtr_marker_label* labels, uint32_t n_labels,
                                    const uint32_t* vals, uint32_t n_vals, const mtr_marker_query* q, uint32_t n,
                                    mtr_marker_hit* out) {
    HIPCHK(hipSetDevice(e->device));
    const std::string name = "mtr_find_markers: ";
    static_assert(sizeof(mtr_marker_label) == 12 && sizeof(mtr_marker_query) == 24 &&
                      sizeof(mtr_marker_hit) == 4 * kHitWords,
                  "layout");
    if ((n_labels && !labels) || (n_vals && !vals) || (n && (!q || !out))) {
        set_err(name + "labels, vals, queries and out are required");
        return -1;
    }
    for (uint32_t j = 0; j < n_labels; j++) {
        const mtr_marker_label& l = labels[j];
        const char* what = uint64_t(l.first) + l.count > n_vals ? "values past n_vals" : nullptr;
        for (uint32_t k = 1; !what && k < l.count; k++)
            if (vals[l.first + k] <= vals[l.first + k - 1]) what = "values that do not ascend";
        if (what) {
            set_err(name + what + " in label " + std::to_string(j) + " (values [" + std::to_string(l.first) + ", +" +
                    std::to_string(l.count) + "))");
            return -1;
        }
    }
    for (uint32_t i = 0; i < n; i++) {
        const bool by_id = q[i].mode == MTR_MK_BY_ID;
        const bool mode_ok = by_id || q[i].mode == MTR_MK_PRECEDING || q[i].mode == MTR_MK_FOLLOWING;
        const char* what = q[i].doc >= e->max_docs ? "bad document" : !mode_ok ? "bad mode"
                           : (!by_id && q[i].label >= n_labels) ? "bad label" : nullptr;
        if (what) {
            set_err(name + what + " in query " + std::to_string(i) + " (document " + std::to_string(q[i].doc) +
                    ", mode " + std::to_string(q[i].mode) + ", label " + std::to_string(q[i].label) + ")");
            return -1;
        }
    }
    if (n == 0) return 0;
    // one upload from page-locked memory: the labels, the value ids, the queries
    const size_t N = n, NL = n_labels, NV = n_vals;
    const size_t vals_at = 3 * NL, q_at = vals_at + NV, words = q_at + kHitWords * N, nrows = kHitWords * N + 1;
    mtr_engine::MarkerQueries& w = e->mkquery;
    if (w.h_up.ensure(words) || w.up.ensure(words) || w.rows.ensure(nrows) || w.h_rows.ensure(nrows)) return -1;
    if (NL) std::memcpy(w.h_up.p, labels, NL * sizeof(mtr_marker_label));
    if (NV) std::memcpy(w.h_up.p + vals_at, vals, NV * sizeof(uint32_t));
    std::memcpy(w.h_up.p + q_at, q, N * sizeof(mtr_marker_query));
    KParams P;
    query_params(e, P);
    int32_t* dflag = w.rows.p + kHitWords * N;
    HIPCHK(hipMemcpyAsync(w.up.p, w.h_up.p, words * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(dflag, 0, sizeof(int32_t), e->stream));
    marker_find_kernel<<<n, NT, lds_bytes_global_mode(int(P.segcap)), e->stream>>>(
        P, reinterpret_cast<const mtr_marker_label*>(w.up.p), w.up.p + vals_at,
        reinterpret_cast<const mtr_marker_query*>(w.up.p + q_at), e->dkind.p, w.rows.p, dflag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w.h_rows.p, w.rows.p, nrows * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (w.h_rows.p[kHitWords * N]) {
        set_err(name + "reference outside the property arena");
        return -1;
    }
    std::memcpy(out, w.h_rows.p, N * sizeof(mtr_marker_hit));
    return n;
}

extern "C" int64_t mtr_get_deltas_batch(mtr_engine* e, const uint32_t* docs, uint32_t n, mtr_delta* out, int64_t cap,
                                        int64_t* doc_first, uint32_t* props, int64_t props_cap, int64_t* props_off) {
    HIPCHK(hipSetDevice(e->device));
    if (n && !doc_first) {
        set_err("mtr_get_deltas_batch: doc_first is required");
        return -1;
    }
    for (uint32_t i = 0; i < n; i++)  // (a null list names documents 0 .. n - 1: the first bad one is max_docs)
        if ((docs ? docs[i] : i) >= e->max_docs) {
            set_err("mtr_get_deltas_batch: bad document " + std::to_string(docs ? docs[i] : i) + " at index " +
                    std::to_string(i));
            return -1;
        }
    if (n == 0) {
        if (doc_first) doc_first[0] = 0;
        if (props_off) props_off[0] = 0;
        return 0;
    }
    if (!out && props_off) {
        set_err("mtr_get_deltas_batch: props_off needs the records (out is null: a size query)");
        return -1;
    }
    const size_t N = n;
    if (!e->has_delta) {  // (the last batch recorded nothing: every count is 0, and there is nothing to read)
        std::memset(doc_first, 0, (N + 1) * sizeof(int64_t));
        if (props_off) props_off[0] = 0;
        return 0;
    }
    mtr_engine::DeltaQueries& w = e->dquery;
    const size_t noff = 2 * N + 3;
    if ((docs && w.list.ensure(N)) || w.len.ensure(2 * N) || w.off.ensure(noff) || w.flag.ensure(1)) return -1;
    if (docs) HIPCHK(hipMemcpyAsync(w.list.p, docs, N * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    const uint32_t* list = docs ? w.list.p : nullptr;
    HIPCHK(hipMemsetAsync(w.flag.p, 0, sizeof(int32_t), e->stream));
    // len = [words | records], so that off = [word offsets (n + 1) | doc_first (n + 1) | flag] and the read-back is one
    // run: the word total, doc_first, the flag
    uint64_t* wcnt = w.len.p;
    uint64_t* cnt = w.len.p + N;
    const mtr_delta* delta = reinterpret_cast<const mtr_delta*>(e->delta.p);
    const uint32_t per = kDeltaThreads / 64;
    const uint32_t grid = uint32_t((N + per - 1) / per);
    delta_count_kernel<<<grid, kDeltaThreads, 0, e->stream>>>(e->hdr.p, list, n, e->n_docs, e->doff.p, delta, e->dkind.p,
                                                             e->prop.p, e->caps.prop_words, props_off != nullptr, wcnt,
                                                             cnt, w.flag.p);
    HIPCHK(hipGetLastError());
    query_scan_kernel<<<1, kScanThreads, 0, e->stream>>>(wcnt, cnt, n, w.flag.p, w.off.p);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> h(N + 3);  // off[n .. 2 n + 2]
    HIPCHK(hipMemcpyAsync(h.data(), w.off.p + N, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (h[N + 2]) {
        set_err(h[N + 2] & kBadHeader ? "mtr_get_deltas_batch: a document's header holds more records than its slice"
                                      : "mtr_get_deltas_batch: reference outside the property arena");
        return -1;
    }
    const int64_t words = h[0], total = h[N + 1];
    std::memcpy(doc_first, h.data() + 1, (N + 1) * sizeof(int64_t));
    if (!out) return total;
    if (cap < total) return MTR_SUMMARY_TOO_SMALL;
    const bool too_small = props_off && props && props_cap < words;
    if (props_off) props_off[total] = words;
    const bool get_recs = !too_small && total > 0;
    const bool get_poff = props_off && total > 0;
    const bool get_props = props_off && props && !too_small && words > 0;
    if (get_recs || get_poff) {
        const size_t T = size_t(total);
        if ((get_recs && w.recs.ensure(T)) || (get_poff && w.poff.ensure(T)) || (get_props && w.props.ensure(size_t(words))))
            return -1;
        delta_records_kernel<<<grid, kDeltaThreads, 0, e->stream>>>(
            list, n, w.off.p + N + 1, w.off.p, e->doff.p, reinterpret_cast<const uint4*>(e->delta.p), e->dkind.p,
            e->prop.p, e->caps.prop_words, get_recs ? reinterpret_cast<uint4*>(w.recs.p) : nullptr,
            get_poff ? w.poff.p : nullptr, get_props ? w.props.p : nullptr);
        HIPCHK(hipGetLastError());
        if (get_recs) HIPCHK(hipMemcpyAsync(out, w.recs.p, T * sizeof(mtr_delta), hipMemcpyDeviceToHost, e->stream));
        if (get_poff) HIPCHK(hipMemcpyAsync(props_off, w.poff.p, T * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
        if (get_props)
            HIPCHK(hipMemcpyAsync(props, w.props.p, size_t(words) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return too_small ? MTR_SUMMARY_TOO_SMALL : total;
}
