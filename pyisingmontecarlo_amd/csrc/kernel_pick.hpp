// Runtime values to template arguments, once for every launcher of the *_kernels.hip units (host code only, no HIP):
//
//   pick(vec, or_last<8, 4, 2>{lpq}, one_of<3, 4, 5, 6>{degree}, [&](auto V, auto L, auto D) { ... kernel<V.value, L.value, D.value> ... });
//
// calls the callable exactly once, with one tag per choice in the order of the choices, or not at all:
//   bool                a flag: std::bool_constant<b>
//   one_of<A, B, ...>   std::integral_constant<int, v> for a v of the list; any other v: no call, pick() returns false
//   or_last<A, ..., Z>  the same, but any v outside the list takes Z
// A choice is a chain of compares in the order of its list, as the if-ladders it stands for: no tables, nothing allocated.  The
// instantiations of the callable are the Cartesian product of the choices; what depends on another choice (a flag that holds only
// together with a second one, an `if constexpr` on a mode) is decided inside the callable, on the tags.
#pragma once

#include <type_traits>
#include <utility>

namespace isingmc {

template <int... Vs> struct one_of { int v; };
template <int... Vs> struct or_last { int v; };

namespace pick_detail {

template <typename B, typename F> std::enable_if_t<std::is_same_v<B, bool>, bool> choose(B b, F &&f) // (no integer passes for a flag)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

template <int V, int... Vs, typename F> bool choose(one_of<V, Vs...> c, F &&f)
{
    if (c.v == V) return f(std::integral_constant<int, V>{});
    if constexpr (sizeof...(Vs) > 0) return choose(one_of<Vs...>{c.v}, f);
    else return false;
}

template <int V, int... Vs, typename F> bool choose(or_last<V, Vs...> c, F &&f)
{
    if constexpr (sizeof...(Vs) > 0) return c.v == V ? f(std::integral_constant<int, V>{}) : choose(or_last<Vs...>{c.v}, f);
    else return f(std::integral_constant<int, V>{});
}

template <typename... Tags> struct picked { // Tags: what the choices before `c` came to
    template <typename C, typename... Rest> static bool then(C &&c, Rest &&...rest)
    {
        if constexpr (sizeof...(Rest) > 0) return choose(c, [&](auto tag) { return picked<Tags..., decltype(tag)>::then(std::forward<Rest>(rest)...); });
        else return c(Tags{}...), true; // the callable
    }
};

} // namespace pick_detail

template <typename... ChoicesThenCallable> bool pick(ChoicesThenCallable &&...a)
{
    return pick_detail::picked<>::then(std::forward<ChoicesThenCallable>(a)...);
}

} // namespace isingmc
