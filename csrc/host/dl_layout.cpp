// fa_dl.h and fa_limits.h by name, for fastapriori_amd.ops.primitives (ctypes): Python
// reads the device loop's slots, limits and mode bits, DlDesc's fields and DlPost's
// layout, and the kernels' capacity limits and pads from here and keeps no copy of them.
#include <stddef.h>

#include "fa_common.h"
#include "fa_dl.h"
#include "fa_limits.h"

namespace {

using namespace fa;

struct Entry { const char* name; int64_t value; };

#define FA_DL_DESC_FIELDS(X) X(P) X(cnt) X(off) X(rows) X(m) X(n) X(C) X(base)
#define FA_DL_POST_FIELDS(X)                                                                        \
  X(item_map) X(rec) X(part) X(out) X(rec_cap) X(part_cap) X(out_cap) X(roff) X(ranks) X(src)       \
  X(wword) X(ncols) X(lds_kernel) X(lds_budget) X(c1) X(alive) X(len_hist) X(T) X(nnz)              \
  X(trim_min_rows) X(trim_ok) X(k) X(done) X(sw) X(cap) X(n_wg) X(C) X(trim) X(gpre) X(gpre_cap)    \
  X(accb) X(trim_rows_frac) X(trim_nnz_frac)

const Entry kLayout[] = {
#define FA_DL_X(name, value) {#name, value},
    FA_DL_CONSTS(FA_DL_X)
#undef FA_DL_X
    {"sizeof(DlDesc)", sizeof(DlDesc)},
#define FA_DL_X(f) {"DlDesc." #f, offsetof(DlDesc, f)},
    FA_DL_DESC_FIELDS(FA_DL_X)
#undef FA_DL_X
    {"sizeof(DlPost)", sizeof(DlPost)},
#define FA_DL_X(f) {"DlPost." #f, offsetof(DlPost, f)},
    FA_DL_POST_FIELDS(FA_DL_X)
#undef FA_DL_X
};

// every field is 8 bytes wide: a field missing from a list above fails here
#define FA_DL_X(f) +1
static_assert(sizeof(DlDesc) == 8 * (0 FA_DL_DESC_FIELDS(FA_DL_X)), "FA_DL_DESC_FIELDS lists every field");
static_assert(sizeof(DlPost) == 8 * (0 FA_DL_POST_FIELDS(FA_DL_X)), "FA_DL_POST_FIELDS lists every field");
#undef FA_DL_X

const Entry kLimits[] = {
#define FA_LIMITS_X(name, value) {#name, value},
    FA_LIMITS_INT(FA_LIMITS_X) FA_LIMITS_U32(FA_LIMITS_X)
#undef FA_LIMITS_X
};

template <int N>
const char* entry(const Entry (&table)[N], int i, int64_t* value) {
  if (i < 0 || i >= N) return nullptr;
  *value = table[i].value;
  return table[i].name;
}

}  // namespace

// Entry i of a table: its name (nullptr past the end) and, in *value, its value
FA_API const char* fa_dl_layout(int i, int64_t* value) { return entry(kLayout, i, value); }
FA_API const char* fa_limits(int i, int64_t* value) { return entry(kLimits, i, value); }
