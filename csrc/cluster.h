// Entry points the clustering sources share: cluster_scatter.hip (intrinsic scores) and clustering.hip (EMI) define them,
// cluster_pairs.hip (extrinsic scores) calls them.
#pragma once

#include "common.h"

namespace tmx {

// labels: any integer dtype [N] -> (inv int32 [N], info int32 {K, wide}); with wide set inv is not written (cluster_scatter.hip)
std::tuple<at::Tensor, at::Tensor> cluster_label_ranks(const at::Tensor& labels);

// a: fp64 [R] row marginals, b: fp64 [K] column marginals; returns the fp64 EMI scalar (clustering.hip)
at::Tensor expected_mutual_info(const at::Tensor& a, const at::Tensor& b, double n_samples);

}  // namespace tmx
