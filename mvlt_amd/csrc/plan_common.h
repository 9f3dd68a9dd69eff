// What the host-only plan headers (gemm_plan.h, attn_plan.h) need of common.h when they are compiled WITHOUT it (a host compiler alone, no HIP):
// the return codes and MVLT_REQUIRE.  Inside the HIP translation units common.h has defined them already and this header adds nothing.
#pragma once
#ifndef MVLT_OK
#define MVLT_OK 0
#define MVLT_ERR_ARG -1
#define MVLT_ERR_UNSUPPORTED -3
void mvlt_set_error(const char* fmt, ...);
#define MVLT_REQUIRE(cond, ...)                 \
  do {                                          \
    if (!(cond)) {                              \
      mvlt_set_error(__VA_ARGS__);              \
      return MVLT_ERR_ARG;                      \
    }                                           \
  } while (0)
#endif
