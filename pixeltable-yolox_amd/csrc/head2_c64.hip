// head_pred2 for 64 feature channels, both 16-bit dtypes (see head2.hpp)
#include "head2.hpp"

namespace yxh {
YXH_HEAD2_UNIT(64);
}  // namespace yxh
