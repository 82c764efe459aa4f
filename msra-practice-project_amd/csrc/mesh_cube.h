// mesh_cube.h - the per-cube "face walk" of marching cubes (mesh_stages.hip), host- and device-callable.
//
// Corner b of a cube = (dx, dy, dz) with b = dx*4 + dy*2 + dz, dx along the volume's first (slowest) axis.
// Edge e = axis*4 + (bits of the two other coordinates, higher axis last): axis 0 -> dy*2+dz, axis 1 -> dx*2+dz,
// axis 2 -> dx*2+dy.  A corner is "in" when its value is above the level (v > level; a corner AT the level is out).
//
// The iso-polygon boundary of a cube is fixed by the corner signs, the crossings and the resolution of every
// ambiguous (checkerboard) face.  Each face, walked counter-clockwise as seen from outside the cube, gives one
// directed segment per out->in crossing, ending at the in->out crossing that closes the region around it; on an
// ambiguous face the asymptotic decider (the sign of the bilinear saddle, a0*a2 - a1*a3) picks the pairing, as
// Lewiner's marching cubes does.  Every crossing is the start of one segment and the end of one, so the segments
// chain into at most 4 loops; each loop of m crossings is fan-triangulated into m-2 triangles.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#endif

namespace mi {
namespace mc {

// corners of face f = axis*2 + side, counter-clockwise seen from outside (outward normal = (2*side-1) e_axis)
__host__ __device__ __forceinline__ int face_corner(int f, int k) {
    const int a = f >> 1, side = f & 1;
    const int u = (a + 1) % 3, w = (a + 2) % 3;
    // (u, w) cycle (0,0) (1,0) (1,1) (0,1) is CCW about +e_a; the -e_a face walks it backwards
    const int ku = side ? k : (4 - k) & 3;
    const int cu = (ku == 1 || ku == 2), cw = (ku >= 2);
    int c[3];
    c[a] = side; c[u] = cu; c[w] = cw;
    return c[0] * 4 + c[1] * 2 + c[2];
}

// the cube edge joining corners p and q (which differ in one coordinate)
__host__ __device__ __forceinline__ int edge_of(int p, int q) {
    const int d = p ^ q;
    const int lo = p & q;
    const int x = (lo >> 2) & 1, y = (lo >> 1) & 1, z = lo & 1;
    if (d == 4) return 0 * 4 + y * 2 + z;
    if (d == 2) return 1 * 4 + x * 2 + z;
    return 2 * 4 + x * 2 + y;
}

// low corner of edge e and its axis
__host__ __device__ __forceinline__ int edge_corner(int e) {
    const int a = e >> 2, b0 = (e >> 1) & 1, b1 = e & 1;
    if (a == 0) return b0 * 2 + b1;
    if (a == 1) return b0 * 4 + b1;
    return b0 * 4 + b1 * 2;
}

struct Loops {
    int n_loops;
    int len[4];
    int8_t edge[12];      // loop l occupies edge[start(l) .. start(l)+len[l])
};

// a[b] = value(corner b) - level, in fp64.  Returns the number of triangles (s - 2l).
__host__ __device__ __forceinline__ int cube_loops(const double a[8], Loops& L) {
    int mask = 0;
    for (int b = 0; b < 8; ++b) mask |= (a[b] > 0.0) << b;
    L.n_loops = 0;
    if (mask == 0 || mask == 255) return 0;
    int8_t next[12];
    for (int e = 0; e < 12; ++e) next[e] = -1;
    for (int f = 0; f < 6; ++f) {
        int c[4], in[4];
        for (int k = 0; k < 4; ++k) { c[k] = face_corner(f, k); in[k] = (mask >> c[k]) & 1; }
        const int n_in = in[0] + in[1] + in[2] + in[3];
        if (n_in == 0 || n_in == 4) continue;
        // face edge k joins c[k] -> c[k+1]
        if (n_in == 2 && in[0] == in[2]) {
            // checkerboard: the saddle is above the level when a0*a2 > a1*a3 (in corners = the positive ones)
            const double s = a[c[0]] * a[c[2]] - a[c[1]] * a[c[3]];
            const int k0 = in[0] ? 0 : 1;          // the two in corners are k0 and k0+2
            const bool joined = in[0] ? (s > 0.0) : (s < 0.0);
            int e[4];
            for (int k = 0; k < 4; ++k) e[k] = edge_of(c[k], c[(k + 1) & 3]);
            // edge k is in->out when corner k is in; out->in when corner k+1 is in
            if (!joined) {
                // cut off each in corner i: segment (edge i-1, out->in) -> (edge i, in->out)
                next[e[(k0 + 3) & 3]] = (int8_t)e[k0];
                next[e[(k0 + 1) & 3]] = (int8_t)e[(k0 + 2) & 3];
            } else {
                // cut off each out corner j = k0+1, k0+3: segment (edge j, out->in) -> (edge j-1, in->out)
                next[e[(k0 + 1) & 3]] = (int8_t)e[k0];
                next[e[(k0 + 3) & 3]] = (int8_t)e[(k0 + 2) & 3];
            }
            continue;
        }
        int start = -1, end = -1;
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            if (in[k] && !in[k1]) end = edge_of(c[k], c[k1]);
            if (!in[k] && in[k1]) start = edge_of(c[k], c[k1]);
        }
        next[start] = (int8_t)end;
    }
    int seen = 0, pos = 0, tris = 0;
    for (int e0 = 0; e0 < 12; ++e0) {
        if (next[e0] < 0 || ((seen >> e0) & 1)) continue;
        int m = 0, e = e0;
        do {
            seen |= 1 << e;
            L.edge[pos + m++] = (int8_t)e;
            e = next[e];
        } while (e != e0);
        L.len[L.n_loops++] = m;
        pos += m;
        tris += m - 2;
    }
    return tris;
}

}  // namespace mc
}  // namespace mi
