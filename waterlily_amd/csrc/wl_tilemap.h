// wl_tilemap.h -- which tile a workgroup of a z-marching launch takes, stated ONCE in plain integer logic: the kernels
// (k_stencil7, k_rowvec, k_correct3, k_convdiff3s, the statistics kernels) call tile_of on the device, the launchers ask
// tilemap_dealt on the host, and tests/tilemap_host.cpp drives both on the host.  Nothing of HIP is included here.
//
// A launch has nblk workgroups = nchunk z-chunks x tpp tiles of the (x,y) plane; logical tile lb = ch*tpp + pt is tile pt
// of chunk ch.  Hardware deals the workgroups round-robin over the 8 XCDs (b and b+8 share an L2), so physical workgroup b
// is the (b>>3)-th workgroup of XCD b&7.  Two maps b -> lb:
//   contiguous  XCD x takes the tiles [x*per, (x+1)*per), per = nblk/8, in order: one contiguous slab of z per XCD;
//   dealt       XCD x takes the chunks x, x+8, x+16, ... in order, each chunk's tpp tiles consecutively: a chunk still
//               sits on one XCD (y-neighbouring tiles share their halo rows through one L2), but consecutive chunks sit on
//               different XCDs, so rows that cost more than the others -- the body's -- are spread over all eight.
// `rev`: every XCD walks its own list of tiles backwards (sweep_rev, wl_common.h).
// The slot of a tile's reduction partial is the same function of lb under both maps and both directions (the workgroup that
// takes the tile in the contiguous map with rev = 0), so every sum adds the same partials in the same order.
#pragma once
#ifndef WL_HD
#if defined(__HIPCC__)
#define WL_HD __host__ __device__ __forceinline__
#else
#define WL_HD inline
#endif
#endif

namespace wl {

// does tile_of(., nblk, tpp, ...) deal chunks?  tpp = 0 asks for the contiguous map; a launch whose chunks do not divide
// evenly among the XCDs (the small sub-range launches of z-slab runs, coarse levels) keeps it too
WL_HD bool tilemap_dealt(int nblk, int tpp) {
    return tpp > 0 && nblk > 0 && !(nblk & 7) && nblk % tpp == 0 && !((nblk / tpp) & 7);
}
// slot of logical tile lb's partial
WL_HD int tile_slot(int lb, int nblk) {
    if (nblk & 7) return lb;
    const int per = nblk >> 3;
    return ((lb % per) << 3) | (lb / per);
}
// logical tile of physical workgroup b, and the slot of that tile's partial
WL_HD void tile_of(int b, int nblk, int tpp, int rev, int &lb, int &pslot) {
    if (nblk & 7) { lb = b; pslot = b; return; }
    const int per = nblk >> 3, x = b & 7, q = b >> 3;
    const int qq = rev ? per - 1 - q : q;
    if (!tilemap_dealt(nblk, tpp)) {
        lb = x * per + qq;
        pslot = (qq << 3) | x;
        return;
    }
    const int c = qq / tpp;                    // the XCD's c-th chunk is chunk x + 8c
    lb = (x + 8 * c) * tpp + (qq - c * tpp);
    pslot = tile_slot(lb, nblk);
}

}  // namespace wl
