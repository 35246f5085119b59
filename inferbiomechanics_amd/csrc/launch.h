// Host-side dispatch of an entry point's storage dtype (and vector width), or of its activation, onto a kernel template.
#pragma once
#include <type_traits>

#include "ib_common.h"
#include "launch_geom.h"

static inline bool ib_dtype_known(int dtype) { return dtype == IB_F32 || dtype == IB_BF16; }

// launch(tag) with a float or a bf16_t value, `using T = decltype(tag)` being the element type: IB_E_DTYPE -- nothing
// launched -- for any other dtype, IB_E_LAUNCH when the launch failed
template <typename F>
static inline int ib_dispatch_dtype(int dtype, F&& launch) {
  if (dtype == IB_F32) launch(float{});
  else if (dtype == IB_BF16) launch(bf16_t{});
  else return IB_E_DTYPE;
  IB_CHECK_LAUNCH();
  return IB_OK;
}

// f(tag) with std::integral_constant<int, IB_ACT_...>, `decltype(tag)::value` being a kernel's activation argument, and
// f's value handed back.  A code outside IB_ACT_RELU .. IB_ACT_ELU runs as IB_ACT_NONE: the entry points refuse unknown
// codes before they dispatch.
template <typename F>
static inline auto ib_dispatch_act(int act, F&& f) {
  switch (act) {
    case IB_ACT_RELU: return f(std::integral_constant<int, IB_ACT_RELU>{});
    case IB_ACT_TANH: return f(std::integral_constant<int, IB_ACT_TANH>{});
    case IB_ACT_SIGMOID: return f(std::integral_constant<int, IB_ACT_SIGMOID>{});
    case IB_ACT_SILU: return f(std::integral_constant<int, IB_ACT_SILU>{});
    case IB_ACT_ELU: return f(std::integral_constant<int, IB_ACT_ELU>{});
    default: return f(std::integral_constant<int, IB_ACT_NONE>{});
  }
}

// a vector width as a type: `decltype(width)::value` is a kernel's template argument
template <int V> using ib_width = std::integral_constant<int, V>;

// launch(tag, width): ib_width<W> when `wide`, ib_width<1> otherwise
template <int W, typename F>
static inline int ib_dispatch_dtype_width(int dtype, bool wide, F&& launch) {
  return ib_dispatch_dtype(dtype, [&](auto tag) {
    if (wide) launch(tag, ib_width<W>{}); else launch(tag, ib_width<1>{});
  });
}
