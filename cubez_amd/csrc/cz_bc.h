// cz_bc.h -- the boundary faces of the global box, stated once for the driver, both multigrid hierarchies and every
// fill of face layers: the state as set, one level's packed word, and the fill's kinds from that word.  Plain C++, no HIP.
#ifndef CZ_BC_H_
#define CZ_BC_H_

// The state as set: nm bit f = face X-, X+, Y-, Y+, Z-, Z+ is a zero-flux (Neumann) face; per bit d = direction X, Y, Z is periodic.  The two
// halves are kept as given: the Neumann flags of a periodic direction stay, ignored while it is periodic (mg_level_bc)
struct CzBc {
  int nm = 0, per = 0;
  CzBc() = default;
  CzBc(int nm_bits, int per_bits) : nm(nm_bits & 63), per(per_bits & 7) {}
  // this state with one half replaced from a setter's argument (faces[6] / dirs[3]: any non-zero flag sets its bit)
  CzBc with_faces(const int* faces) const {
    int v = 0;
    for (int f = 0; f < 6; f++) v |= faces[f] ? 1 << f : 0;
    return CzBc(v, per);
  }
  CzBc with_dirs(const int* dirs) const { return CzBc(nm, (dirs[0] ? 1 : 0) | (dirs[1] ? 2 : 0) | (dirs[2] ? 4 : 0)); }
  bool any() const { return (nm | per) != 0; }
};

namespace czhip_internal {
// One level's packed word (MgdLevel::nm, MgLev::nm: bits 0 .. 5 the mask, bits 6 .. 8 the wraps) from the state that was set (nm: the six
// Neumann flags, per: bit d = direction d is periodic) and the level's global points gn.  In a periodic direction the Neumann flags are
// ignored; a level of two or more points there wraps (bit 6 + d), a level of one point has no link in that direction -- the point's
// neighbours are itself -- and takes both mask bits (c = 0) and no wrap.  per = 0: nm itself, at every level
inline int mg_level_bc(int nm, int per, const int* gn) {
  int v = 0;
  for (int d = 0; d < 3; d++) {
    if (!((per >> d) & 1)) v |= nm & (3 << (2 * d));
    else if (gn[d] < 2) v |= 3 << (2 * d);
    else v |= 64 << d;
  }
  return v;
}
inline int mg_level_bc(CzBc s, const int* gn) { return mg_level_bc(s.nm, s.per, gn); }

// The fill's kinds[6] (0 leave, 1 mirror, 2 wrap; czhip_fill_faces_async) for an array of a level with packed word `word`.  mirrors: the array
// carries its Neumann faces as mirrored face layers -- level 0 and the driver's arrays; at levels >= 1 the masked diagonal carries them
inline void bc_kinds(int* kinds, int word, bool mirrors) {
  for (int f = 0; f < 6; f++) kinds[f] = (word >> (6 + (f >> 1))) & 1 ? 2 : (mirrors && ((word >> f) & 1)) ? 1 : 0;
}
}  // namespace czhip_internal

#endif
