// tree_id.hip -- git tree ids of the summary trees on the device (mtr_summary_tree_ids / mtr_git_tree_ids).
//
// A tree's id is SHA-1("tree " + decimal body length + NUL + body); the body is the entries sorted by name (a
// subtree comparing as its name + '/') and concatenated, each "<mode in octal> <name>\0" + the 20 raw id bytes
// (what `git mktree` hashes; what storage answers createGitTree with).
//
// SHA-1 is serial within one object, so the parallelism is across trees, one lane per tree in every kernel:
//   tree_size_kernel   walks the tree's entries in sorted order and adds their sizes up (arithmetic only)
//   (scan_u32_launch)  the blob table's single-workgroup exclusive scan turns sizes into offsets
//   tree_write_kernel  the same walk, now storing each entry's bytes: the bodies back to back in one byte buffer
//   git_tree_id_kernel git_object_id (git_object_id.hip.h: the blob kernel's loader and 80 rounds) over each body
// Materialising the body keeps the hashing kernel's 16-word window statically indexed (no scratch; build.py refuses a
// build with any): entry bytes pushed into w[i] with a runtime i would put the window in memory.
//
// The two walks are one function (walk_tree<WRITE>), so the sizes and the writes cannot disagree; the write pass
// also stops at the tree's end offset, so no store leaves [off[t], off[t + 1]).
#include "tree_id.hip.h"

#include "blob_id.hip.h"
#include "git_object_id.hip.h"

namespace mtr {

namespace {

// The sort key of a name: its first 16 bytes big-endian in two words, zero-padded, a subtree's name followed by '/'.
// Names hold no NUL, so comparing keys compares names bytewise; an engine-made name has at most 15 bytes, so its key
// ends in a zero byte and 16 bytes decide every comparison with it.
struct Key {
    uint64_t hi, lo;
};
__device__ __forceinline__ void key_put(Key& k, uint32_t pos, uint32_t c) {
    if (pos < 8) k.hi |= uint64_t(c) << (56 - 8 * pos);
    else k.lo |= uint64_t(c) << (56 - 8 * (pos - 8));
}
__device__ __forceinline__ uint32_t key_byte(const Key& k, uint32_t pos) {
    return uint32_t((pos < 8 ? k.hi >> (56 - 8 * pos) : k.lo >> (56 - 8 * (pos - 8))) & 0xff);
}
__device__ __forceinline__ bool key_less(const Key& a, const Key& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

constexpr uint64_t kBody = 0x626f6479ull;           // "body"
constexpr uint64_t kHeader = 0x686561646572ull;     // "header"
constexpr uint64_t kSegments = 0x7365676d656e7473ull;  // "segments"

// "body_<k in decimal>"
__device__ __forceinline__ Key body_key(uint32_t k, uint32_t& name_len) {
    Key key{(kBody << 32) | (uint64_t('_') << 24), 0};
    uint32_t digits = 1;
    for (uint32_t x = k; x >= 10; x /= 10) digits++;
    uint32_t x = k;
    for (uint32_t j = digits; j-- > 0;) {
        key_put(key, 5 + j, '0' + x % 10);
        x /= 10;
    }
    name_len = 5 + digits;
    return key;
}

// the successor of cur among the decimal strings of [1, max] in bytewise order (cur is not the last of them)
__device__ __forceinline__ uint32_t lex_next(uint32_t cur, uint32_t max) {
    if (uint64_t(cur) * 10 <= max) return cur * 10;
    while (cur % 10 == 9 || cur >= max) cur /= 10;
    return cur + 1;
}

struct Sink {
    uint8_t* p;
    uint32_t pos, end;
};
template <bool WRITE>
__device__ __forceinline__ void put(Sink& s, uint32_t c) {
    if (WRITE && s.pos < s.end) s.p[s.pos] = uint8_t(c);
    s.pos++;
}
template <bool WRITE>
__device__ __forceinline__ void put_mode(Sink& s, bool tree) {
    if (WRITE) {
        // "100644 " or "40000 "
        if (tree) {
            put<true>(s, '4');
            for (int j = 0; j < 4; j++) put<true>(s, '0');
        } else {
            put<true>(s, '1');
            put<true>(s, '0');
            put<true>(s, '0');
            put<true>(s, '6');
            put<true>(s, '4');
            put<true>(s, '4');
        }
        put<true>(s, ' ');
    } else {
        s.pos += tree ? 6 : 7;
    }
}
// an engine-made entry: the name is the key's bytes, the id five words
template <bool WRITE>
__device__ __forceinline__ void put_engine(Sink& s, const Key& k, uint32_t name_len, bool tree, const uint32_t* id) {
    put_mode<WRITE>(s, tree);
    if (WRITE) {
        for (uint32_t j = 0; j < name_len; j++) put<true>(s, key_byte(k, j));
        put<true>(s, 0);
        for (int j = 0; j < 5; j++) {
            const uint32_t v = id[j];
            for (int q = 0; q < 4; q++) put<true>(s, (v >> (8 * q)) & 0xff);
        }
    } else {
        s.pos += name_len + 21;
    }
}
__device__ __forceinline__ bool is_tree(const mtr_tree_entry& x) { return x.mode == 040000u; }
template <bool WRITE>
__device__ __forceinline__ void put_extra(Sink& s, const mtr_tree_entry& x) {
    put_mode<WRITE>(s, is_tree(x));
    if (WRITE) {
        for (uint32_t j = 0; j < x.name_len && j < MTR_TREE_NAME_MAX; j++) put<true>(s, uint8_t(x.name[j]));
        put<true>(s, 0);
        for (int j = 0; j < 20; j++) put<true>(s, x.id[j]);
    } else {
        s.pos += uint32_t(x.name_len) + 21;
    }
}
__device__ __forceinline__ Key extra_key(const mtr_tree_entry& x) {
    Key k{0, 0};
    const uint32_t nl = x.name_len;  // (1..MTR_TREE_NAME_MAX: name[j] below stays inside the 39-byte field)
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t c = j < nl ? uint8_t(x.name[j]) : (j == nl && is_tree(x) ? uint32_t('/') : 0u);
        key_put(k, j, c);
    }
    return k;
}

// Tree t of the job, entry by entry in sorted order; returns the body's size.  WRITE: stores the bytes at
// body[off[t] ..), never at or past off[t + 1].
template <bool WRITE>
__device__ __forceinline__ uint32_t walk_tree(const TreeJob& J, uint32_t t) {
    Sink s{J.body, 0, 0};
    if (WRITE) {
        s.pos = J.off[t];
        s.end = J.off[t + 1];
    }
    const uint32_t start = s.pos;
    const bool vec = J.first && J.kind && J.kind[t] != 0;
    uint32_t b0 = 0, nb = 0;
    if (J.first) {
        b0 = J.first[t];
        nb = J.first[t + 1] - b0;
    }
    if (J.level == 1 && (!vec || nb == 0)) return 0;  // (no outer tree: the hashing kernel skips it too)
    // the engine-made entries as a sequence in sorted order: n_eng of them, e_* the current one
    uint32_t n_eng, chunks = 0;
    if (J.level == 1) {
        n_eng = 2;  // handleTable, then segments
    } else {
        n_eng = vec ? (nb ? nb - 1 : 0) : nb;  // header + chunks
        chunks = n_eng ? n_eng - 1 : 0;
    }
    uint32_t xi = 0, xn = 0;
    if (J.x_first && !(J.level == 0 && vec)) {
        xi = J.x_first[t];
        xn = J.x_first[t + 1];
    }
    uint32_t ei = 0, cur = 0;  // cur: the chunk number of engine entry ei (v1)
    Key ek{0, 0}, xk{0, 0};
    uint32_t e_len = 0;
    bool e_tree = false;
    const uint32_t* e_id = nullptr;
    auto load_engine = [&]() {
        if (ei >= n_eng) return;
        if (J.level == 1) {
            if (ei == 0) {
                ek = Key{0x68616e646c655461ull, 0x626c650000000000ull};  // "handleTable"
                e_len = 11;
                e_tree = false;
                e_id = J.blob_ids + 5 * (size_t(b0) + nb - 1);
            } else {
                ek = Key{kSegments, uint64_t('/') << 56};
                e_len = 8;
                e_tree = true;
                e_id = J.out + 5 * size_t(t);
            }
            return;
        }
        e_tree = false;
        if (ei == chunks) {  // the last: "header" (blob 0) sorts after every "body..."
            ek = Key{kHeader << 16, 0};
            e_len = 6;
            e_id = J.blob_ids + 5 * size_t(b0);
        } else if (J.v1) {   // "body_<cur>" (blob 1 + cur), cur running through [0, chunks) in string order
            cur = ei == 0 ? 0 : (ei == 1 ? 1 : lex_next(cur, chunks - 1));
            ek = body_key(cur, e_len);
            e_id = J.blob_ids + 5 * (size_t(b0) + 1 + cur);
        } else {             // legacy: "body" (blob 1 + ei; the engine refuses a legacy record with more than one)
            ek = Key{kBody << 32, 0};
            e_len = 4;
            e_id = J.blob_ids + 5 * (size_t(b0) + 1 + ei);
        }
    };
    load_engine();
    if (xi < xn) xk = extra_key(J.x[xi]);
    while (ei < n_eng || xi < xn) {
        const bool take_x = ei >= n_eng || (xi < xn && key_less(xk, ek));
        if (take_x) {
            put_extra<WRITE>(s, J.x[xi]);
            xi++;
            if (xi < xn) xk = extra_key(J.x[xi]);
        } else {
            put_engine<WRITE>(s, ek, e_len, e_tree, e_id);
            ei++;
            load_engine();
        }
    }
    return s.pos - start;
}

__global__ void __launch_bounds__(256) tree_size_kernel(TreeJob J) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= J.n) return;
    J.off[t] = walk_tree<false>(J, t);
}

__global__ void __launch_bounds__(256) tree_write_kernel(TreeJob J) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= J.n) return;
    (void)walk_tree<true>(J, t);
}

}  // namespace

// One lane per tree over the materialised bodies.  body is 4-byte aligned and holds the total rounded up to 4, so
// the aligned words git_object_id loads (those holding at least one body byte) lie inside it.  Level 1 hashes the
// outer trees of matrix vector documents only (skip: the kinds), leaving the other documents' ids as level 0 made them.
constexpr int kTreeIdThreads = 64;  // one wave per workgroup: a workgroup ends with its longest tree
__global__ void __launch_bounds__(kTreeIdThreads) __attribute__((amdgpu_waves_per_eu(8)))
git_tree_id_kernel(const uint8_t* __restrict__ body, const uint32_t* __restrict__ off, uint32_t n,
                   const uint32_t* __restrict__ first, const uint32_t* __restrict__ skip, uint32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if (skip && (skip[t] == 0 || first[t + 1] == first[t])) return;
    const uint32_t o = off[t];
    git_object_id(kGitTypeTree, uintptr_t(body) + o, off[t + 1] - o, out + 5 * size_t(t));
}

hipError_t tree_ids_launch(const TreeJob& job, hipStream_t s) {
    if (job.n == 0) return hipSuccess;
    const uint32_t groups = (job.n + 255) / 256;
    tree_size_kernel<<<groups, 256, 0, s>>>(job);
    hipError_t rc = scan_u32_launch(job.off, job.n, s);
    if (rc != hipSuccess) return rc;
    tree_write_kernel<<<groups, 256, 0, s>>>(job);
    // (level 1 without kinds has no outer trees: the walk sized every tree 0, and every lane is skipped)
    const uint32_t* skip = job.level == 1 ? job.kind : nullptr;
    if (job.level == 1 && !skip) return hipGetLastError();
    git_tree_id_kernel<<<(job.n + kTreeIdThreads - 1) / kTreeIdThreads, kTreeIdThreads, 0, s>>>(job.body, job.off, job.n,
                                                                                               job.first, skip, job.out);
    return hipGetLastError();
}

}  // namespace mtr
