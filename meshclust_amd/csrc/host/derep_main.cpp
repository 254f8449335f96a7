// derep_main.cpp -- bin/meshclust-derep (derep_run.hpp).  Exit codes as meshclust-assign's: a usage
// error is 1 with the usage text, an unreadable file or no reads 2.
#ifdef _OPENMP
#include <omp.h>
#endif

#include "derep_run.hpp"

int main(int argc, char **argv) {
  using namespace mc;
  try {
    const DerepOptions opt = parse_derep_options(argc, argv);
#ifdef _OPENMP
    if (opt.threads > 0) omp_set_num_threads(opt.threads);
#endif
    const DerepResult r = run_derep(nullptr, opt);
    if (!opt.quiet)
      printf("%llu reads: %llu unique (%llu written), largest class %llu, %llu on the minus strand\n", (unsigned long long)r.reads,
             (unsigned long long)r.uniques, (unsigned long long)r.written, (unsigned long long)r.largest, (unsigned long long)r.minus);
    if (!opt.stats_json.empty()) {
      if (FILE *f = fopen(opt.stats_json.c_str(), "w")) {
        fprintf(f, "%s\n", derep_stats_json(r).c_str());
        fclose(f);
      }
    }
    return 0;
  } catch (const Error &e) {
    fprintf(stderr, "%s\n", e.what());
    return e.code ? e.code : 1;
  } catch (const std::exception &e) {
    fprintf(stderr, "meshclust-derep: %s\n", e.what());
    return 1;
  }
}
