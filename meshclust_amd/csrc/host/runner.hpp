// runner.hpp -- the meshclust driver: options (Runner::get_opts, src/cluster/src/Runner.cpp:
// 150-263), k choice (find_k :265-292), histogram width dispatch (run :41-90) and the
// do_run pipeline (:321-375), on top of the libmcgpu C-ABI.
#pragma once
#include <string>
#include <vector>

#include "cluster.hpp"
#include "common.hpp"
#include "fasta.hpp"
#include "trainer.hpp"

namespace mc {

struct Options {
  int k = -1;
  double similarity = 0.90;
  int iterations = 15;
  int delta = 5;
  bool align = false;
  int sample_size = 0;
  int pivots = 20;
  int threads = 0;  // 0 = OpenMP default
  std::string output = "output.clstr";
  std::vector<std::string> files;
  // additions of this implementation
  int device = 0;
  std::vector<int> devices;  // --devices 0,1,..: one clustering shared by these GPUs (RCCL)
  bool quiet = false;
  std::string stats_json;  // per-phase timings + work counts
  std::string save_model;    // --save-model FILE: k, id, the trained classifier (model.hpp)
  std::string save_centres;  // --save-centres FILE: the final centres as FASTA, cluster order
  // --both-strands: cluster on canonical rows (row[i] + row[rc(i)] - 1), so a read and its reverse
  // complement are the same point; --strands FILE: every member's strand against its centre
  bool both_strands = false;
  std::string strands_file;
};

// Parses argv like the reference; bad input throws mc::Error (OptionError in runner.cpp)
// with the reference's message and exit code.
Options parse_options(int argc, char **argv, bool require_files = true);

struct RunResult {
  std::vector<Center> part;
  PhaseTimer timer;
  ClusterStats stats;
  int k = 0;
  int width = 1;
  uint64_t largest = 0;
  size_t n = 0;
  // what read assignment needs beside the centres (model.hpp): the trained classifier and the
  // options as the pipeline resolved them
  mc_classifier cls{};
  double similarity = 0;
  bool align = false;
  // --both-strands: strands 3, the doubled mean length the automatic k was computed from, and per
  // cluster (rr.part order) every member's strand against its centre (mc_orient_pairs: 0 plus,
  // 1 minus) with sad_plus / sad_minus interleaved
  int strands = 1;
  uint64_t k_auto_length = 0, members_minus = 0;
  std::vector<std::vector<uint8_t>> member_strand;
  std::vector<std::vector<uint64_t>> member_sad;
};

// Runner::find_k's formula (Runner.cpp:265-292) on a mean length: ceil(log4(length)) - 1.
int recommended_k(unsigned long long length);

// --strands FILE of a finished --both-strands run: one line per read in .clstr order,
// name, cluster, centre name, + or -, sad_plus, sad_minus (tab separated; a name is the header
// line without '>', as in meshclust-assign's TSV)
void write_strands_file(const std::string &path, const Dataset &ds, const RunResult &rr);

// --save-model / --save-centres of a finished run (where the .clstr is written; rank 0 only).
void save_model_files(const Options &opt, const Dataset &ds, const RunResult &rr);

// Full pipeline on an already parsed dataset and an open context (bench.py reuses both).
bool tune_host_heap();  // process-global malloc settings (runner.cpp); true when applied
RunResult run_pipeline(const Dataset &ds, mc_ctx *ctx, Options opt, bool upload = true,
                       const ShardComm *comm = nullptr);

// JSON summary of a run (phase timings, work counts) for --stats-json and the C API.
std::string stats_json(const RunResult &rr, double parse_ms, double write_ms);

int meshclust_main(int argc, char **argv);

}  // namespace mc
