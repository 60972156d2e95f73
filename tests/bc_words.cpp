// bc_words.cpp -- cz_bc.h on the host alone (tests/test_bc_words.py compiles and runs it): for every state (64 Neumann masks x 8 periodic sets)
// and every level of 1, 2 or 5 points per direction one line
//   nm per gx gy gz : word : kinds[6] of an array that mirrors its Neumann faces : kinds[6] of one that does not
#include <cstdio>

#include "cz_bc.h"

int main() {
  const int ext[3] = {1, 2, 5};
  for (int nm = 0; nm < 64; nm++)
    for (int per = 0; per < 8; per++) {
      int faces[6], dirs[3];
      for (int f = 0; f < 6; f++) faces[f] = (nm >> f) & 1 ? 1 + f : 0;  // (any non-zero flag sets the face)
      for (int d = 0; d < 3; d++) dirs[d] = (per >> d) & 1 ? -1 - d : 0;
      const CzBc s = CzBc().with_faces(faces).with_dirs(dirs);
      if (s.nm != nm || s.per != per || s.any() != (nm || per)) return 1;
      for (int a = 0; a < 27; a++) {
        const int gn[3] = {ext[a / 9], ext[a / 3 % 3], ext[a % 3]};
        const int word = czhip_internal::mg_level_bc(s, gn);
        printf("%d %d %d %d %d : %d :", nm, per, gn[0], gn[1], gn[2], word);
        for (int mirrors = 1; mirrors >= 0; mirrors--) {
          int kinds[6];
          czhip_internal::bc_kinds(kinds, word, mirrors != 0);
          for (int f = 0; f < 6; f++) printf(" %d", kinds[f]);
          printf(mirrors ? " :" : "\n");
        }
      }
    }
  return 0;
}
