// Stand-alone driver of the dense kernel's decisions in grand_plus_amd/csrc/gfpush_plan.hpp for tests/test_host_dense.py.  One
// query per line on stdin:
//   consts                                                      -> kDenseMaxNodes kDenseLds kDenseCtlBytes kDenseHistBytes
//   wanted kernel n_nodes nnz n_coef rmax K lds_pad              -> 0 | 1
//   plan n_nodes nnz K lds_pad dn_block dn_csr_lds num_cus per_cu max_workgroups n_seeds
//        -> fits csr_lds lds_bytes block workgroups n_pad off_hist off_cur off_next off_reserve off_marks off_indptr off_indices state_end
// Built with the address and undefined-behaviour sanitizers; no HIP, no GPU.
#include "gfpush_plan.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace gp::planning;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "consts") {
            std::printf("%lld %d %d %d\n", (long long)kDenseMaxNodes, kDenseLds, kDenseCtlBytes, kDenseHistBytes);
        } else if (what == "wanted") {
            Options opt; long long n = 0, nnz = 0; int n_coef = 0, K = 0, pad = 0; double rmax = 0.0;
            if (!(in >> opt.kernel >> n >> nnz >> n_coef >> rmax >> K >> pad)) { std::fprintf(stderr, "bad query: %s\n", line.c_str()); return 2; }
            opt.lds_pad = pad;
            std::printf("%d\n", dense_wanted(opt, n, nnz, n_coef, rmax, K, pad) ? 1 : 0);
        } else if (what == "plan") {
            Options opt; long long n = 0, nnz = 0, n_seeds = 0; int K = 0, pad = 0, cus = 0, per_cu = 0;
            if (!(in >> n >> nnz >> K >> pad >> opt.dn_block >> opt.dn_csr_lds >> cus >> per_cu >> opt.max_workgroups >> n_seeds)) {
                std::fprintf(stderr, "bad query: %s\n", line.c_str());
                return 2;
            }
            opt.kernel = 3; opt.lds_pad = pad;
            const DensePlan d = dense_plan(opt, n, nnz, K, pad, cus, per_cu, n_seeds);
            std::printf("%d %d %d %d %d %lld %u %u %u %u %u %u %u %u\n", d.fits ? 1 : 0, d.csr_lds ? 1 : 0, d.lds_bytes, d.block, d.workgroups,
                        (long long)d.n_pad, d.off_hist, d.off_cur, d.off_next, d.off_reserve, d.off_marks, d.off_indptr, d.off_indices, d.state_end);
        } else {
            std::fprintf(stderr, "bad query: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
