// In-kernel time stamps of the diagnostic build (build.sh diag: every unit with -DUBD_STAMPS, tools/_ab/libubd_hip_diag.so).  The product
// build sees only the empty macros at the end (arguments are not evaluated): no kernel parameter, no global, no exported symbol.
//
// Host: tools register one (buffer, capacity in 64-bit words, two selectors) entry per kernel family through the one exported setter
//   ubd_debug_set_stamps(kernel, buf, capacity_words, sel0, sel1)                                     (api.hip; buf == nullptr clears the entry)
// and a launch site appends UBD_STAMP_ARG("family"[, sel0[, sel1]]) to its argument list: the family's buffer where the selectors it names
// are the registered ones, else an empty one.  Families and their selectors: the table in api.hip.
// Device: a stamped kernel ends its parameter list with UBD_STAMP_PARAM and writes through UBD_STAMP(cond, index) (s_memtime, the CU's shader
// clock) or UBD_STAMP_RT (s_memrealtime, the 100-MHz clock all CUs share: block time lines): lane 0 of every wave for which `cond` holds
// stores the clock to word `index` -- only where a buffer is set and index < capacity, so a buffer that does not match a kernel's grid loses
// stamps instead of writing out of bounds.  Each kernel keeps its index expression and its "first N tiles" guard in a macro of its own.
#pragma once
#ifdef UBD_STAMPS
struct ubd_stamp_buf { unsigned long long *p; size_t cap; };
ubd_stamp_buf ubd_stamps_for(const char *kernel, int sel0 = 0, int sel1 = 0);
#define UBD_STAMP_PARAM , ubd_stamp_buf stamps = {}
#define UBD_STAMP_ARG(...) , ubd_stamps_for(__VA_ARGS__)
#define UBD_STAMPS_ONLY(...) __VA_ARGS__
#define UBD_STAMP_CLOCK(clock, cond, index) do { if (stamps.p && (threadIdx.x & 63) == 0 && (cond)) { const size_t i_ = (size_t)(index); if (i_ < stamps.cap) stamps.p[i_] = clock(); } } while (0)
#define UBD_STAMP(cond, index) UBD_STAMP_CLOCK(__builtin_amdgcn_s_memtime, cond, index)
#define UBD_STAMP_RT(cond, index) UBD_STAMP_CLOCK(__builtin_amdgcn_s_memrealtime, cond, index)
#else
#define UBD_STAMP_PARAM
#define UBD_STAMP_ARG(...)
#define UBD_STAMPS_ONLY(...)
#define UBD_STAMP(cond, index) do {} while (0)      // a statement, as in the diagnostic build (not nothing: clang numbers a function's jump
#define UBD_STAMP_RT(cond, index) do {} while (0)   // targets, and a kernel's loop-exit selectors in registers carry those numbers)
#endif
