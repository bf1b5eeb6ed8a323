// mpcekf_pack.hpp -- series strings along the fused loop (mpcekf_pack_begin): the record's
// rows, the kernel's arguments and the launches of mpcekf_pack.hip.  Not a reference function:
// runMPC.m charges one cell; a pack string carries one current, the one its weakest cell accepts.
#pragma once

#include <cstdint>

namespace mk {

// rows of the record [NPKR][n], in the order of include/mpcekf.h's MPCEKF_PK_* (checked in
// mpcekf_host.cpp)
enum { PK_NLIM = 0, PK_STEPS, PK_HEADROOM, NPKR };

// strings no longer than this share a block of PACK_BLOCK lanes; longer ones get a block each
constexpr int PACK_BLOCK = 256;

struct KPack {
  double *uk, *uk_1;  // [n] s.uk: each cell's command, replaced by the string current; s.uk_1 likewise
  double *u;          // [n] this step's u row of the call's outputs, may be null
  double *ucmd;       // [n] this step's row of the commands before the reduction, may be null
  int *limiter;       // [n / series] this step's row of in-string limiter indices, may be null
  double *rec;        // [NPKR][n]
  int64_t n;
  int series;         // cells per string; n % series == 0
};

// one step's coupling, after the step's Hildreth (and k_cl_diag), before the summary fold and
// k_thermal
int launch_pack(const KPack &q, void *stream);

}  // namespace mk
