// The one RBF element expression of the SVM kernels (xps_svm.hip: rbf_from_gram_kernel; xps_svm_cv.hip: rbf_multi_from_gram_kernel):
// libsvm's exp(-gamma (x.x + y.y - 2 x.y)) from a Gram element g and the two squared norms.  Both kernels call this function, so a
// matrix of the multi-gamma kernel equals the single-gamma kernel's bit for bit.  (2 g is exact, so the distance rounds once
// whether or not the compiler contracts it into an FMA; the product with gamma and the exp are the same operations.)
#pragma once

__device__ inline double xps_rbf_from_gram(double gamma, double na, double nb, double g) { return exp(-gamma * (na + nb - 2.0 * g)); }
