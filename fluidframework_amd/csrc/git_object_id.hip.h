// git_object_id.hip.h -- the id of one git object on one lane: SHA-1("<type> " + decimal byte length + NUL + the
// bytes).  Device code shared by git_blob_id_kernel (blob_id.hip, type "blob") and git_tree_id_kernel (tree_id.hip,
// type "tree"); both object types have four letters, so only the first prefix word differs.
//
// SHA-1 is a serial chain within one object, so the parallelism is across objects: one lane per object, each lane
// streaming its own 64-byte blocks.  Lanes of a wave run different numbers of blocks; the block loop holds no
// cross-lane operation and no barrier, so the divergent trip count is safe.  The 80 rounds are fully unrolled: the
// 16-word schedule window is indexed statically and stays in VGPRs (no scratch; fluidframework_amd/build.py refuses
// a build of either kernel with any).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mtr {

constexpr uint32_t kGitTypeBlob = 0x626c6f62u;  // "blob"
constexpr uint32_t kGitTypeTree = 0x74726565u;  // "tree"

__device__ __forceinline__ uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

// one SHA-1 compression; w is consumed (the schedule is computed in place)
__device__ __forceinline__ void sha1_block(uint32_t (&h)[5], uint32_t (&w)[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
    for (int t = 0; t < 80; t++) {
        uint32_t wt;
        if (t < 16) {
            wt = w[t];
        } else {
            wt = rotl(w[(t - 3) & 15] ^ w[(t - 8) & 15] ^ w[(t - 14) & 15] ^ w[t & 15], 1);
            w[t & 15] = wt;
        }
        uint32_t f, k;
        if (t < 20) {
            f = d ^ (b & (c ^ d));
            k = 0x5a827999u;
        } else if (t < 40) {
            f = b ^ c ^ d;
            k = 0x6ed9eba1u;
        } else if (t < 60) {
            f = (b & c) | (d & (b | c));
            k = 0x8f1bbcdcu;
        } else {
            f = b ^ c ^ d;
            k = 0xca62c1d6u;
        }
        const uint32_t tmp = rotl(a, 5) + f + e + k + wt;
        e = d;
        d = c;
        c = rotl(b, 30);
        b = a;
        a = tmp;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
}

// The message of object (src, len) is: the prefix "<type> <len>\0" (P = 7..16 bytes), the content, 0x80, zeros, and
// the 64-bit big-endian bit count, in 64-byte blocks.  The content is never block-aligned (P varies with the digit
// count) and src has any byte alignment, so content words come from aligned 32-bit loads funnel-shifted by
// (address & 3).  Only aligned words holding at least one byte of the object are loaded (none when len is 0).
// id receives the 20 id bytes as five words.
__device__ __forceinline__ void git_object_id(uint32_t type_word, uintptr_t src, uint32_t len, uint32_t* id) {
    // the prefix as four big-endian words, zero after its P bytes: the type, then ' ' + digits + NUL left-aligned
    // in 96 bits (built from the last digit: each step shifts a byte in at the top)
    uint32_t pw[4] = {type_word, 0, 0, 0};
    uint32_t P = 6;
    {
        uint32_t x = len;
        do {
            const uint32_t q = x / 10u, c = '0' + (x - 10u * q);
            pw[3] = (pw[3] >> 8) | (pw[2] << 24);
            pw[2] = (pw[2] >> 8) | (pw[1] << 24);
            pw[1] = (pw[1] >> 8) | (c << 24);
            x = q;
            P++;
        } while (x);
        pw[3] = (pw[3] >> 8) | (pw[2] << 24);
        pw[2] = (pw[2] >> 8) | (pw[1] << 24);
        pw[1] = (pw[1] >> 8) | (uint32_t(' ') << 24);
    }
    const uint64_t total = uint64_t(P) + len;            // message bytes before the padding
    const uint64_t bits = total * 8;                     // (a u32 length times 8 needs 64 bits)
    const uint32_t n_blocks = uint32_t((total + 9 + 63) >> 6);
    uint32_t h[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
    for (uint32_t blk = 0; blk < n_blocks; blk++) {
        // block-relative byte positions: the content covers [s_rel, e_rel), the 0x80 byte sits at p80
        const int64_t k0 = int64_t(uint64_t(blk) << 6) - int64_t(P);  // content offset of the block's first byte
        const int64_t rem = int64_t(len) - k0;                        // content bytes from there on (any sign)
        const int s_rel = blk == 0 ? int(P) : 0;
        const int e_rel = rem < s_rel ? s_rel : (rem > 64 ? 64 : int(rem));
        const int p80 = (rem >= 0 && rem < 64) ? int(rem) : -64;
        // the block's bytes lie in the aligned words ap[0 .. 16] (the 17th only when sh != 0); word j holds the
        // block-relative bytes [4j - sh, 4j - sh + 4), so the words with content are [lo_w, hi_w)
        const uintptr_t a = uintptr_t(int64_t(src) + k0);
        const uint32_t sh = uint32_t(a) & 3u;
        const uint32_t* ap = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
        const int lo_w = (s_rel + int(sh)) >> 2;
        const int hi_w = e_rel > s_rel ? ((e_rel - 1 + int(sh)) >> 2) + 1 : 0;
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = (j >= lo_w && j < hi_w) ? ap[j] : 0u;
        const uint32_t x16 = hi_w > 16 ? ap[16] : 0u;
#pragma unroll
        for (int j = 0; j < 16; j++)
            w[j] = __builtin_bswap32(__builtin_amdgcn_alignbyte(j < 15 ? w[j + 1] : x16, w[j], sh));
        if (s_rel != 0 || e_rel != 64) {
            // a block holding the prefix, the content's end, the padding or the bit count: mask the bytes outside
            // the content off, then OR in what the prefix, the 0x80 byte and the bit count put there
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int lo_cut = min(max(s_rel - 4 * j, 0), 4), hi_cut = min(max(4 * j + 4 - e_rel, 0), 4);
                uint32_t v = w[j] & uint32_t(0xffffffffull >> (8 * lo_cut)) & uint32_t(0xffffffffull << (8 * hi_cut));
                const int r = p80 - 4 * j;
                if (r >= 0 && r < 4) v |= 0x80u << (24 - 8 * r);
                if (j < 4 && blk == 0) v |= pw[j];
                w[j] = v;
            }
            if (blk == n_blocks - 1) {
                w[14] |= uint32_t(bits >> 32);
                w[15] |= uint32_t(bits);
            }
        }
        sha1_block(h, w);
    }
#pragma unroll
    for (int j = 0; j < 5; j++) id[j] = __builtin_bswap32(h[j]);
}

}  // namespace mtr
