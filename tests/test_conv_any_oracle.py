"""The cases of tests/test_resnet_any_gpu.py checked on the float64
references alone, without a GPU: that the integer cases are exact in the
kernels' arithmetic and are not tests of zeros, that the damages a subtly
wrong kernel would do change every reference, that the chunk-spanning wgrad
cases span chunks, and that the random-valued bound K = 4 * 2.57 still
covers float32 CPU convolutions over this geometry list.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import conv_oracle as co  # noqa: E402
import conv_any_oracle as ca  # noqa: E402

TWO24 = 2.0 ** 24
ALL_GEOMS = ca.GEOMS + tuple(g for g, _ in ca.WGRAD_CHUNK_CASES
                             if g not in ca.GEOMS)


def _is_int(t):
    return bool((t == t.round()).all())


def _kinds(geom):
    return ("fwd", "dgrad", "wgrad") if ca.has_dgrad(geom) else ("fwd",
                                                                 "wgrad")


@pytest.mark.parametrize("geom", ALL_GEOMS)
def test_integer_cases_are_exact_and_covered(geom):
    ci, h, w, c_out = geom
    c = ca.int_case(geom)
    assert _is_int(c["x"]) and _is_int(c["dy"])
    assert float(c["x"].abs().max()) <= 2 and float(c["dy"].abs().max()) <= 2
    for yy in (0, -1):
        for xx in (0, -1):
            assert bool((c["x"][:, yy, xx, :] != 0).all())
    for n in ca.NS:
        for kind in _kinds(geom):
            r = ca.refs(geom, kind, n)
            s = ca.refs(geom, kind, n, True, True)
            for name, ref in r.items():
                assert _is_int(ref), f"{geom} {name} N={n}"
                assert float(s[name].max()) < TWO24
                if name in co.BF16_OUT:
                    assert float(ref.abs().max()) <= 256
                share = float((ref != 0).double().mean())
                print(f"SHARE {geom} {name} N={n}: {share:.3f}, max"
                      f" {float(ref.abs().max()):.0f}, S"
                      f" {float(s[name].max()):.0f}")
                assert share < 0.80, f"{geom} {name} N={n}: {share:.3f}"
                if (h, w) != (1, 1):
                    assert share > 0.25, f"{geom} {name} N={n}: {share:.3f}"
    dw = ca.refs(geom, "wgrad", 1)["dW"]
    assert dw.shape == (3, c_out, co.kwcp(3, ci))
    assert not bool(dw[..., 3 * ci:].any())


def _differs(a, b):
    return any(not torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("geom", [g for g in ALL_GEOMS
                                  if g[1] >= 3 and g[2] >= 3])
def test_mutations_change_every_reference(geom):
    """Each damage of conv_oracle.py must show in the reference of each
    case, or a kernel doing that damage would pass on it."""
    n = ca.NMAX
    ops = ca.int_ops(geom, n)
    for kind in _kinds(geom):
        entry = ca.ENTRY[kind]
        ref = ca.refs(geom, kind, n)

        def through(m_ops):
            return co.entry_refs(entry, m_ops)

        if kind == "wgrad":
            mutants = dict(
                m_row=through(co.mutate_m_row(entry, ops)),
                neighbour_in=through(co.mutate_neighbour_in(entry, ops)))
        else:
            mutants = dict(tap=through(co.mutate_tap(entry, ops)),
                           neighbour_out=co.mutate_neighbour_out(ref))
        mutants["edge"] = through(co.mutate_edge(entry, ops))
        for name, got in mutants.items():
            assert _differs(got, ref), f"{geom} {kind}: {name} changes nothing"


@pytest.mark.parametrize("geom,n", ca.WGRAD_CHUNK_CASES)
def test_wgrad_chunk_cases_span_chunks(geom, n):
    m = n * geom[1] * geom[2]
    mc, nchunks = ca.wgrad_chunk(m)
    assert n <= ca.NMAX and nchunks >= 2 and m % 64 != 0 and mc % 64 == 0


def test_chunk_cases_cover_every_channel_pair():
    pairs = {(g[0], g[3]) for g, _ in ca.WGRAD_CHUNK_CASES}
    assert pairs == {(8, 16), (16, 16), (16, 32), (32, 16), (32, 32)}


def test_cpu_float32_ratio_within_recorded():
    """The random-valued cases are held to co.K = 4 r with the project's
    r = 2.57; float32 on the CPU over this list must stay inside r, so a
    changed generator cannot loosen the bound unnoticed."""
    worst = ca.cpu_float32_ratio()
    print("float32 CPU vs float64, units of 2^-24*S:",
          {k: round(v, 3) for k, v in worst.items()},
          f"recorded r = {co.CPU_RATIO}, K = {co.K:.2f}")
    assert max(worst.values()) <= co.CPU_RATIO
