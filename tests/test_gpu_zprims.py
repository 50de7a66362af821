"""The vector primitives of the complex factorisation on the device (csrc/zfac.hip: k_zdotc_partial / k_zdotc_final,
k_zabsmax_partial / k_zabsmax_final, k_zscale_copy, k_zupdate, the transfers) through tests/zprim_checks.py: a recording callback
operator turns mispec_zfac_init into a probe of each primitive against numpy.longdouble, with Higham's gamma_k bounds counted from
the kernels' source.  The sizes sit on the edges of the fixed partition: 2048-row chunks (2047 / 2048 / 2049, 4097), one
wavefront / one workgroup (63 / 64, 255 / 256 / 257), the 256 chunks one pass of the final kernel covers (524 287 / 524 288 /
524 289) and the benchmark's size (10^7 + 3: 4883 chunks, 20 passes).  Single steps of the general flow over a dense device
operator cover X^H y and the update for every column count up to 40 (groups of 8 columns: 8 | 9, 16 | 17).  The same module runs on
a host backend in tests/test_host_zprims.py."""
import pytest

import spectra_amd as sa

import zprim_checks as P

pytestmark = [pytest.mark.gpu, pytest.mark.operator_only]


@pytest.mark.parametrize("n", P.PROBE_SIZES)
def test_probe_of_the_reductions_and_the_update(ctx, n):
    P.run_probe(sa.lib(), ctx.h, n, P.hip_dot_roundings)


@pytest.mark.parametrize("n,m", P.STEP_SHAPES)
def test_single_steps_over_a_dense_device_operator(ctx, n, m):
    P.run_steps(sa.lib(), ctx.h, n, m)
