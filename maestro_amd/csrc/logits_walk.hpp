// The walk over resident head logits in patch layout that the confusion kernels (metrics.hip) and the prediction kernels
// (predict.hip) share: how the [n_rows, ld] matrix is cut into tiles of whole pixels, how a tile is staged in LDS, and the one
// statement of the arg-max rule both take.
#pragma once
#include "common.hpp"

constexpr int CF_THREADS = 256;
constexpr int CF_TILE = 4096;             // floats of one staged logits tile (16 KiB): 4 16-byte loads per thread
constexpr int CF_VEC = CF_TILE / 4 / CF_THREADS;
constexpr int CF_MAX_PIX = 1024;          // pixels of one tile at most (small C)

// How the [n_rows, ld] logits are cut into tiles, in memory order.  A row holds PP = P * P pixels of C floats.  PP <= npt: a tile is
// `rows_per_tile` whole rows; otherwise a tile is one chunk of `npt` pixels (a multiple of 4: every chunk starts on a 16-byte
// boundary of its row) of one row, the last chunk of a row shorter.
struct CfGeom {
    long n_rows, n_tiles;
    int g, P, C, Cs, ld, PP, npt, rows_per_tile, chunks_per_row, vec;
};

struct CfTile {
    long row0;      // first logits row
    int nr;         // rows
    int pix0;       // first pixel inside the row(s)
    int pps;        // pixels per row segment; the segment is n = pps * C floats from column pix0 * C
};

// The geometry of one call.  `whole_passes`: a tile of more than CF_THREADS pixels is cut down to a multiple of CF_THREADS, so that
// the one-thread-per-pixel scan has no mostly idle last pass (the prediction kernels; the confusion kernels keep the larger tile).
static inline CfGeom cf_geometry(const float* logits, long n_rows, int g, int P, int C, int ld, bool whole_passes) {
    CfGeom G;
    G.n_rows = n_rows;
    G.g = g; G.P = P; G.C = C; G.Cs = C | 1; G.ld = ld; G.PP = P * P;
    G.npt = min(CF_MAX_PIX, CF_TILE / G.Cs) & ~3;      // >= 28 (C = 128)
    if (whole_passes && G.npt > CF_THREADS) G.npt &= ~(CF_THREADS - 1);
    if (G.PP <= G.npt) {
        G.rows_per_tile = G.npt / G.PP;
        G.chunks_per_row = 1;
        G.n_tiles = (G.n_rows + G.rows_per_tile - 1) / G.rows_per_tile;
    } else {
        G.rows_per_tile = 1;
        G.chunks_per_row = (G.PP + G.npt - 1) / G.npt;
        G.n_tiles = G.n_rows * G.chunks_per_row;
    }
    // 16-byte loads: every row and every chunk start on a 16-byte boundary, and a tile of several rows has whole vectors per row
    G.vec = ((uintptr_t)logits % 16 == 0 && ld % 4 == 0 && (G.rows_per_tile == 1 || (G.PP * C) % 4 == 0)) ? 1 : 0;
    return G;
}

__device__ __forceinline__ CfTile cf_tile(const CfGeom& G, long t) {
    CfTile T;
    if (G.chunks_per_row == 1) {
        T.row0 = t * G.rows_per_tile;
        T.nr = (int)min((long)G.rows_per_tile, G.n_rows - T.row0);
        T.pix0 = 0;
        T.pps = G.PP;
    } else {
        T.row0 = t / G.chunks_per_row;
        const int ch = (int)(t - T.row0 * G.chunks_per_row);
        T.nr = 1;
        T.pix0 = ch * G.npt;
        T.pps = min(G.npt, G.PP - T.pix0);
    }
    return T;
}

// Local element e of a tile (rows concatenated, pad columns left out) -> its address.
__device__ __forceinline__ const float* cf_addr(const float* logits, const CfGeom& G, const CfTile& T, unsigned e) {
    const unsigned n = (unsigned)T.pps * G.C, r = e / n, o = e - r * n;
    return logits + (size_t)(T.row0 + r) * G.ld + (size_t)T.pix0 * G.C + o;
}

// Element e goes to tile[(e / C) * Cs + e % C]: Cs = C | 1 is odd, so the 64 lanes that each scan one pixel hit 64 different banks.
__device__ __forceinline__ void cf_stage4(float* tile, const CfGeom& G, unsigned e, const f32x4 v) {
    unsigned p = e / G.C, c = e - p * G.C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        tile[p * G.Cs + c] = v[j];
        if (++c == (unsigned)G.C) { c = 0; ++p; }
    }
}

// The 16-byte loads of one tile into registers (issued a tile ahead), and their way into the LDS tile.
struct CfPrefetch {
    f32x4 v[CF_VEC];
    float tail;
};

__device__ __forceinline__ void cf_prefetch(CfPrefetch& pre, const float* logits, const CfGeom& G, const CfTile& T, int tid) {
    const unsigned total = (unsigned)T.nr * T.pps * G.C, nvec = total >> 2, tail = total & 3;
#pragma unroll
    for (int k = 0; k < CF_VEC; ++k) {
        const unsigned i = tid + k * CF_THREADS;
        if (i < nvec) pre.v[k] = *reinterpret_cast<const f32x4*>(cf_addr(logits, G, T, i * 4));
    }
    if ((unsigned)tid < tail) pre.tail = *cf_addr(logits, G, T, nvec * 4 + tid);
}

// Tile T into LDS: from the prefetched registers (vec), or element by element from memory.
__device__ __forceinline__ void cf_stage(float* tile, const CfPrefetch& pre, const float* logits, const CfGeom& G, const CfTile& T,
                                         int tid) {
    const unsigned total = (unsigned)T.nr * T.pps * G.C;
    const int C = G.C;
    if (G.vec) {
        const unsigned nvec = total >> 2, tail = total & 3;
#pragma unroll
        for (int k = 0; k < CF_VEC; ++k) {
            const unsigned i = tid + k * CF_THREADS;
            if (i < nvec) cf_stage4(tile, G, i * 4, pre.v[k]);
        }
        if ((unsigned)tid < tail) {
            const unsigned e = nvec * 4 + tid, p = e / C;
            tile[p * G.Cs + (e - p * C)] = pre.tail;
        }
    } else {
        for (unsigned e = tid; e < total; e += CF_THREADS) {
            const unsigned p = e / C;
            tile[p * G.Cs + (e - p * C)] = *cf_addr(logits, G, T, e);
        }
    }
}

// torch.argmax over x[0], x[stride], ..., x[(C - 1) * stride]: the lowest index among equal maxima; a NaN is the maximum and the
// first NaN wins.  `best` receives the winning value.
template <typename Ptr>
__device__ __forceinline__ int argmax_torch(Ptr x, int C, size_t stride, float& best) {
    best = x[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float v = x[c * stride];
        if (v > best || (v != v && best == best)) { best = v; arg = c; }
    }
    return arg;
}
