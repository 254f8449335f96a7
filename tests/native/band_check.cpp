// band_check.cpp -- host/band.hpp (the geometry and the certificate gpu/abi_align.hip plans the
// banded choice record with) printed on a grid, without a GPU and without either library;
// tests/test_band_host.py holds every line against the Python formulas of tests/band_cases.py.
//   G la lb w : ub whole cols steps bytes bnd_ints nblk, then c0 c1 of every block
//   P la lb S : neg_inf above_ninf need plan full_bytes, then certified at w = 0, 1, 7, 64
// Also checked here: every window lies in 1 .. lb, holds its rows' band cells, is no wider than
// band_cols, and starts no earlier than the window above it.  Header only.  Ends with "OK".
#include <cstdio>
#include <initializer_list>

#include "band.hpp"

static int fail(const char *what, long a, long b, long w) {
  printf("FAIL: %s (%ld x %ld, w %ld)\n", what, a, b, w);
  return 1;
}

int main() {
  const long lens[] = {0, 1, 2, 17, 65, 255, 256, 257, 300, 511, 512, 513, 1000, 1024, 1025, 1100, 4000, 10000};
  const long widths[] = {0, 1, 5, 16, 64, 300, 5000, 20000};
  for (long la : lens)
    for (long lb : lens) {
      for (long w : widths) {
        if (la == 0 || lb == 0) continue;
        const long nblk = (la + mc::BAND_ROWS - 1) / mc::BAND_ROWS;
        printf("G %ld %ld %ld : %lld %d %llu %llu %llu %llu %ld", la, lb, w, (long long)mc::band_ub(la, lb, w),
               (int)mc::band_is_whole(la, lb, w), (unsigned long long)mc::band_cols(la, lb, w),
               (unsigned long long)mc::band_steps(la, lb, w), (unsigned long long)mc::band_choice_bytes(la, lb, w),
               (unsigned long long)mc::band_bnd_ints(la, lb, w), nblk);
        const long d = lb - la, dlo = (d < 0 ? d : 0) - w, dhi = (d > 0 ? d : 0) + w;
        long pc0 = 1;
        for (long k = 0; k < nblk; k++) {
          const mc::BandWindow win = mc::band_window(la, lb, w, k);
          printf(" %lld %lld", (long long)win.c0, (long long)win.c1);
          if (win.c0 < 1 || win.c1 > lb || win.c0 > win.c1) return fail("a window outside 1 .. lb", la, lb, w);
          if ((unsigned long long)(win.c1 - win.c0 + 1) > mc::band_cols(la, lb, w)) return fail("a window wider than band_cols", la, lb, w);
          if (win.c0 < pc0) return fail("a window that starts before the one above", la, lb, w);
          pc0 = win.c0;
          const long r0 = k * mc::BAND_ROWS + 1, r1 = la < (k + 1) * mc::BAND_ROWS ? la : (k + 1) * mc::BAND_ROWS;
          for (long i : {r0, r1}) {  // the band cells of the block's first and last row
            const long lo = i + dlo < 1 ? 1 : i + dlo, hi = i + dhi > lb ? lb : i + dhi;
            if (lo <= hi && (lo < win.c0 || hi > win.c1)) return fail("a band cell outside its window", la, lb, w);
          }
        }
        printf("\n");
      }
      const long mn = la < lb ? la : lb, df = la > lb ? la - lb : lb - la;
      for (long S : {mn, mn - 1, mn - df - 4, mn - df - 5, mn - df - 6, mn - df - 7, mn - df - 8, mn - df - 100, mn - df - 1000,
                     (long)mc::band_neg_inf(la, lb) + mn, (long)mc::band_neg_inf(la, lb) + mn + 1, (long)mc::band_neg_inf(la, lb)}) {
        printf("P %ld %ld %ld : %lld %d %lld %d %llu", la, lb, S, (long long)mc::band_neg_inf(la, lb), (int)mc::band_above_ninf(la, lb, S),
               (long long)mc::band_need(la, lb, S), (int)mc::band_plan(la, lb, S), (unsigned long long)mc::full_choice_bytes(la, lb));
        for (long w : {0, 1, 7, 64}) printf(" %d", (int)mc::band_certified(la, lb, w, S));
        printf("\n");
      }
    }
  printf("R %d %d %d\n", mc::BAND_R, mc::BAND_ROWS, mc::BAND_SENTINEL);
  printf("OK\n");
  return 0;
}
