// The one first-maximum reduction of the vote kernels (xps_bagging.hip: bag_vote_kernel; xps_svm_cv.hip: svm_cv_score_kernel):
// libsvm's tie rule, so an ensemble vote and a search's prediction break ties alike.
#pragma once

// first maximum over the 64 lanes of (value, index): the larger value, on equal values the SMALLER index
__device__ inline void wave_first_max(int& v, int& c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ov = __shfl_xor(v, o), oc = __shfl_xor(c, o);
        if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
    }
}
