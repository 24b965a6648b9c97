// sdf_chunk_plan.h -- the host-only arithmetic of the meshing paths through device memory (sdf_chunked.hip): how many batches go
// into one submission, when the soup grows, a batch's box, a shard's slice of the work list, and the `_skip` test around a host
// callback.  Pure C++17 with no HIP header, so that a host test compiles it alone (tests/test_large_batch_host.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

#define SDF_BATCH_SIZE_MAX 512   // (513^3 float32 = 540 MB per tile: one tile per submission there)
// at most this many batches per submission
enum { FIELD_CHUNK_MAX = 32 };

// Tiles per submission: as many (bs + 1)^3 float32 tiles as fit 256 MiB, between 1 and FIELD_CHUNK_MAX -- ONE tile is always taken
// whole.  (The tape path used to say (256 << 20) / (tile * 4), "<= 256 MB of volumes", the callback path (64 << 20) / tile, "<= 64 M
// points = 2 GB of pinned points + values": the same integer for every tile size.)  Row slots per tile (k_field_rows): a row of cells
// each, rounded to the 256 threads of a block; the callback path pins 1024 where a tile has at most 32^2 rows.
struct ChunkPlan { size_t tile; int ch, slots; };   // samples of a whole tile, tiles per submission, row slots per tile
inline ChunkPlan chunk_plan(int bs, bool callback) {
    const size_t tile = (size_t)(bs + 1) * (bs + 1) * (bs + 1);
    return {tile, (int)std::max<size_t>(1, std::min<size_t>(FIELD_CHUNK_MAX, ((size_t)256 << 20) / (tile * 4))),
            callback && bs <= 32 ? 1024 : ((bs * bs + 255) & ~255)};
}

// The soup's growth rule (march_chunk): a chunk of n triangles behind `total` kept ones (72 bytes each) in a soup of cap_bytes.
// Returns the new capacity in bytes -- geometric, 4 MiB at least -- or 0: what is there holds the chunk.
inline size_t soup_growth(size_t cap_bytes, unsigned long long total, unsigned long long n) {
    return (total + n) * 72 <= cap_bytes ? 0 : std::max<size_t>((size_t)(total + n) * 72 * 2, (size_t)1 << 22);
}

// a batch's first sample and its number of samples per axis: the host's copy of batch_origin (sdf_device.h), for batch
// b = (ibx * nby + iby) * nbz + ibz of an nx x ny x nz grid cut into batches of bs cells
struct BatchBox { int ox, oy, oz, lx, ly, lz; };
inline BatchBox batch_box(int nx, int ny, int nz, int bs, int b) {
    const int nby = (ny + bs - 1) / bs, nbz = (nz + bs - 1) / bs;
    const int ibz = b % nbz, iby = (b / nbz) % nby, ibx = b / (nbz * nby);
    BatchBox o;
    o.ox = ibx * bs; o.oy = iby * bs; o.oz = ibz * bs;
    o.lx = std::min(bs + 1, nx - o.ox); o.ly = std::min(bs + 1, ny - o.oy); o.lz = std::min(bs + 1, nz - o.oz);
    return o;
}

// shard i of k takes items [shard_cut(n, i, k), shard_cut(n, i + 1, k)) of a work list of length n: [n * i / k, n * (i + 1) / k), what
// k_compact computes on the device
inline int shard_cut(long long n, long long i, long long k) { return (int)((n * i) / k); }

// `_skip` (reference sdf/core.py:28-43) around a host callback.  skip_points writes the nine points of a batch whose first and
// last samples are (x0, y0, z0) and (x1, y1, z1): the centre, then itertools.product((x0, x1), (y0, y1), (z0, z1)).
inline void skip_points(double x0, double x1, double y0, double y1, double z0, double z1, double *p) {
    p[0] = (x0 + x1) / 2; p[1] = (y0 + y1) / 2; p[2] = (z0 + z1) / 2;
    for (int k = 0; k < 8; k++) {
        p[3 + 3 * k] = (k & 4) ? x1 : x0; p[4 + 3 * k] = (k & 2) ? y1 : y0; p[5 + 3 * k] = (k & 1) ? z1 : z0;
    }
}
// ... and the verdict from the field's values v[0 .. 8] at those points: 0 (skipped) or 255 (pending).  (p + 3 is the first corner.)
inline unsigned char skip_verdict(const double *p, const double *v) {
    const double x0 = p[3], y0 = p[4], z0 = p[5];
    const double r = fabs(v[0]);
    const double d = sqrt(((p[0] - x0) * (p[0] - x0) + (p[1] - y0) * (p[1] - y0)) + (p[2] - z0) * (p[2] - z0));
    bool same = true;
    const bool pos = v[1] > 0.0;
    for (int k = 1; k <= 8; k++) same = same && (pos ? v[k] > 0.0 : v[k] < 0.0);
    return (!(r <= d) && same) ? 0 : 255;
}
