// pr_logstep.hpp — the text and the decisions of pr-learn's log (src/pr-learn.cpp:200-262,364-403), shared by
// pr-learn (one setting, to stdout) and pr-learn-grid (one log file per setting) so that the two cannot differ.
#pragma once

#include <cfloat>
#include <cstdio>
#include <ostream>
#include <string>
#include <vector>

namespace pr_log {

// the first line: the setting and the run's limits
inline void config(std::ostream &o, float mu, float gamma, int MaxDim, unsigned nIter)
{
    o << "mu: " << mu << " gamma: " << gamma << " maxdim: " << MaxDim << " nIters: " << nIter << std::endl;
}

inline void loaded(std::ostream &o, int nDists, int FeatDim)
{
    o << "Load Labels: " << nDists << std::endl;
    o << "Load Distances: " << nDists << " x " << FeatDim << std::endl;
}

// the index split and the device block that precede the first LogStep line
inline void split(std::ostream &o, int n_pos, int n_pos_trn, int n_neg, int n_neg_trn, const char *gpu, int cc_major, int cc_minor)
{
    o << "Positive samples #" << n_pos << std::endl;
    o << "Negative samples #" << n_neg << std::endl;
    o << "Positive train #" << n_pos_trn << std::endl;
    o << "Negative train #" << n_neg_trn << std::endl;
    o << "Positive valid #" << n_pos - n_pos_trn << std::endl;
    o << "Negative valid #" << n_neg - n_neg_trn << std::endl;
    o << std::endl;
    o << "Found GPU: " << gpu << std::endl;
    o << "Compute Capability: " << cc_major << "." << cc_minor << std::endl;
    o << std::endl;
}

// The best objective so far and the w it was reached with (:364-369)
struct Best {
    float Obj_Best = FLT_MAX;
    int nnz_best = 0;
    std::vector<float> w_Best;
};

// The validation line of iteration t.  Returns true for a new best objective: b then holds w, and the
// caller runs the statistics and finishes the entry with stat().
inline bool objective(std::string &out, Best &b, unsigned t, float LossVal, float Regul, int nnz, const float *w, size_t F, double ttime,
                      double vtime)
{
    char line[512];
    const bool best = (LossVal + Regul) < b.Obj_Best;
    if (best) {
        b.Obj_Best = LossVal + Regul;
        b.w_Best.assign(w, w + F);
        b.nnz_best = nnz;
    }
    std::snprintf(line, sizeof(line), "%s: %i  Loss: %.6f Regul: %.6f Obj: %.6f (%.6f)  NNZ: %i (%i)  Ttime: %.4f Vtime: %.4f\n",
                  best ? "Best" : "Step", t, LossVal, Regul, (LossVal + Regul), b.Obj_Best, nnz, b.nnz_best, ttime, vtime);
    out += line;
    return best;
}

// the save rule of a new best (:385): its w is appended to the output when Dim fits MaxDim
inline bool saves(int Dim, int MaxDim) { return Dim <= MaxDim; }

// the statistics line of a new best (:385-403)
inline void stat(std::string &out, int nPR, int nzDim, int Dim, int MaxDim, double AUC, float FPR95, bool saved)
{
    char line[512];
    std::snprintf(line, sizeof(line), "Stat: nPR #%i (#%i) Dim/MaxDim [%i/%i] AUC: %.6f FPR95: %.2f%s\n", nPR, nzDim, Dim, MaxDim, AUC,
                  FPR95 * 100, saved ? " [saved]" : "");
    out += line;
}

}  // namespace pr_log
