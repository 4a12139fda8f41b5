// head_pred2 for 320 feature channels, both 16-bit dtypes (see head2.hpp)
#include "head2.hpp"

namespace yxh {
YXH_HEAD2_UNIT(320);
}  // namespace yxh
