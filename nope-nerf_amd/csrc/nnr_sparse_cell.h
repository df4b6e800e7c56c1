#include "nnr_cell_rule.h"      // the cell rule of include/nnr_sparse.h (sparse_cell), under the name nnr_sparse_f16.hip and nnr_frozen_sparse.hip include
