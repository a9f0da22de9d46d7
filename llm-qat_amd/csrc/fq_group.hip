// fq_group.hip -- instantiations of the group-wise forward (fq_group.h) for the three element types: a translation unit of its own, so
// the row-wise units compile exactly as before and this one builds beside them.
#include "fq_group.h"
namespace fq {
FQ_INSTANTIATE_GROUP(F32)
FQ_INSTANTIATE_GROUP(BF16)
FQ_INSTANTIATE_GROUP(F16)
}
