// qmvt_classify_pair.h -- launcher of k_classify_pair (qmvt_classify_pair.hip): the classification of sorted, single-base,
// column-input batches.  Everything else (packed input of the radix-sort path, allele-extended batches) stays with
// k_classify of qmvt_kernels.hip; launch_classify_any picks.
#pragma once
#include "qmvt_dev.h"

namespace qm {

// needs !P.pkey && !P.ext; writes what k_classify<false, false> writes, bit for bit
void launch_classify_pair(const ClassifyParams& P, int n_spans, hipStream_t st);

// the one place that decides which classification kernel a launch runs
inline void launch_classify_any(const ClassifyParams& P, int n_spans, hipStream_t st) {
  if (!P.pkey && !P.ext) launch_classify_pair(P, n_spans, st);
  else launch_classify(P, n_spans, st);
}

}  // namespace qm
