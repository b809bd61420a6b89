// pr_cli.hpp — what pr-learn and pr-learn-grid do alike before and around the library calls: the flags they share,
// the input files, and the LogStep schedule (src/pr-learn.cpp:78-82,200-262,331,419-422).
#pragma once

#include "dlco_io.hpp"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <ostream>
#include <stdexcept>
#include <vector>

namespace pr_cli {

// The flags both tools take, with the reference's constants as defaults (:80-82,241)
struct CommonFlags {
    int MaxDim = 640;
    unsigned nIter = 5000000, LogStep = 100000;
    unsigned long long seed = 2215;
    int device = 0;

    // true when argv[i] is one of them and has a value: the value is consumed (i moves onto it)
    bool parse(int argc, char **argv, int &i)
    {
        if (i + 1 >= argc) return false;
        const char *a = argv[i];
        if (std::strcmp(a, "-maxdim") == 0) MaxDim = atoi(argv[++i]);
        else if (std::strcmp(a, "-iters") == 0) nIter = (unsigned)atoi(argv[++i]);
        else if (std::strcmp(a, "-logstep") == 0) LogStep = (unsigned)atoi(argv[++i]);
        else if (std::strcmp(a, "-seed") == 0) seed = strtoull(argv[++i], nullptr, 10);
        else if (std::strcmp(a, "-device") == 0) device = atoi(argv[++i]);
        else return false;
        return true;
    }
};

// PRParams of the filter file and Distance / Label of the distance file
struct Inputs {
    std::vector<size_t> pshape;
    std::vector<float> PRParams, dists;
    std::vector<uint8_t> labels;
    int nDists = 0, FeatDim = 0;
};

// Reads and checks the four datasets; with `say`, "Load <name>." goes there before each read of the filter file, as
// the reference prints it
inline Inputs load(const char *flt, const char *src, std::ostream *say)
{
    Inputs in;
    std::vector<size_t> rshape, dshape, lshape;
    std::vector<float> RingParams;
    if (say) *say << "Load PRParams." << std::endl;
    dlco_io::read_dataset<float>(flt, "PRParams", in.pshape, in.PRParams);
    if (say) *say << "Load RingParams." << std::endl;
    dlco_io::read_dataset<float>(flt, "RingParams", rshape, RingParams);          // read like the reference; not used by this stage
    dlco_io::read_dataset<float>(src, "Distance", dshape, in.dists);
    dlco_io::read_dataset<uint8_t>(src, "Label", lshape, in.labels);
    if (dshape.size() != 2 || in.pshape.size() != 2) throw std::runtime_error("Distance and PRParams must be 2-D datasets");
    in.nDists = (int)dshape[0]; in.FeatDim = (int)dshape[1];
    if ((int)in.labels.size() < in.nDists) throw std::runtime_error("Label has fewer rows than Distance");
    if ((int)in.pshape[0] < 8 * in.FeatDim) throw std::runtime_error("PRParams needs 8 rows per column of Distance");
    return in;
}

using Clock = std::chrono::steady_clock;
inline double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// The LogStep schedule.  The reference logs inside iteration t when its step counter has reached LogStep, i.e. at
// t = LogStep, 2 LogStep + ... with `step` restarting from 0 -> every LogStep iterations, the first time after
// LogStep + 1 of them (src/pr-learn.cpp:331,419-422); t runs to nIter inclusive.  run(n) trains n more iterations;
// log(t, train_start) writes the entry of iteration t, train_start being when the window that reached t began (the
// clock restarts after each entry).
template <typename Run, typename Log>
void logstep_schedule(unsigned nIter, unsigned LogStep, Run &&run, Log &&log)
{
    unsigned t_done = 0;                                   // iterations run so far (t = 0 .. t_done-1)
    unsigned long long next_log = LogStep;                 // t of the next entry: LogStep, 2 LogStep, ... (every t >= 1 for LogStep = 1)
    Clock::time_point train_start = Clock::now();
    while (t_done <= nIter) {
        const unsigned upto = next_log <= nIter ? (unsigned)next_log + 1 : nIter + 1;   // run up to and including the next logging iteration
        run(upto - t_done);
        t_done = upto;
        if (next_log > nIter) break;
        log((unsigned)next_log, train_start);
        next_log += LogStep;
        train_start = Clock::now();
    }
}

}  // namespace pr_cli
