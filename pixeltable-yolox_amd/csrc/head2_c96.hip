// head_pred2 for 96 feature channels, both 16-bit dtypes (see head2.hpp)
#include "head2.hpp"

namespace yxh {
YXH_HEAD2_UNIT(96);
}  // namespace yxh
