// batch_dispatch.h -- the one dispatch: run-time properties of a batch -> compile-time constants of a kernel instantiation
// (internal; for the .hip files that launch kernels on a BatchView).
// A launcher names the AXES its kernel is instantiated on and gets, inside RP_DISPATCH's statement,
//   S     storage type in HBM: double (RP_DTYPE_F64) or float (RP_DTYPE_F32, RP_DTYPE_F32_STATE)                       always
//   T     arithmetic type in registers    kArith: double / float / double for the three dtypes
//                                         kDoubleArith: double whatever the dtype (mu_mode 1; rp_batch_set_params refuses it for pure fp32)
//                                         neither: S
//   V, M  variant and its row length      kVariant: 3, 16 or 4, 12; otherwise 3, 16
//   Z     BatchView::zero_end_vel         kZeroVel: as the batch says; otherwise true
// An axis that is not named is not branched on: a kernel is instantiated for the combinations its launchers can reach and no others
// (no MU = 1 in float arithmetic, the transposes on S and M only, k_solution / k_init_const / k_nudge / k_sample_records on S only).
#pragma once

#include <type_traits>

#include "ip_kernels.h"

namespace rp {

namespace {

enum : unsigned { kStorage = 0, kArith = 1, kDoubleArith = 2, kVariant = 4, kZeroVel = 8 };

template <typename S_, typename T_, int V_, bool Z_> struct Tag {
    using S = S_;
    using T = T_;
    static constexpr int V = V_, M = V_ == 4 ? 12 : 16;      // M: state_len(V)
    static constexpr bool Z = Z_;
};

template <unsigned AXES, typename F> void dispatch(const BatchView &b, F f)
{
    auto on_zero_vel = [&](auto s, auto t, auto v) {
        constexpr int V = decltype(v)::value;
        if constexpr ((AXES & kZeroVel) != 0) { if (!b.zero_end_vel) return f(Tag<decltype(s), decltype(t), V, false>{}); }
        f(Tag<decltype(s), decltype(t), V, true>{});
    };
    auto on_variant = [&](auto s, auto t) {
        if constexpr ((AXES & kVariant) != 0) { if (b.variant != 3) return on_zero_vel(s, t, std::integral_constant<int, 4>{}); }
        on_zero_vel(s, t, std::integral_constant<int, 3>{});
    };
    if (b.dtype == 0) on_variant(double{}, double{});
    else if constexpr ((AXES & kDoubleArith) != 0) on_variant(float{}, double{});
    else if constexpr ((AXES & kArith) != 0) { if (b.dtype == 1) on_variant(float{}, float{}); else on_variant(float{}, double{}); }
    else on_variant(float{}, float{});
}

#define RP_DISPATCH(AXES, b, ...)                                         \
    dispatch<(AXES)>((b), [&](auto tag_) {                                \
        using S [[maybe_unused]] = typename decltype(tag_)::S;            \
        using T [[maybe_unused]] = typename decltype(tag_)::T;            \
        [[maybe_unused]] constexpr int V = decltype(tag_)::V, M = decltype(tag_)::M; \
        [[maybe_unused]] constexpr bool Z = decltype(tag_)::Z;            \
        __VA_ARGS__;                                                      \
    })

// where the problems lie, for the kernels that walk problems (slots) and those that walk positions (problems); null: in problem order
inline const uint32_t *slots(const BatchView &b) { return b.scheduled ? b.slot_of : nullptr; }
inline const uint32_t *problems(const BatchView &b) { return b.scheduled ? b.prob_of : nullptr; }

}  // namespace

}  // namespace rp
