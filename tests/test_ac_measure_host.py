"""The AC measurement definition on the CPU: ac_measure_exec.h — the code of the kernel in spicey_amd/csrc/ac_measure.hip —
through the lane emulation of tests/ac_measure_host against reduce_ac_reference (plain numpy).  No field is a sum, so all 8
doubles of every row agree bit for bit, whatever the lane count, the number of waves or the other requests are."""
import numpy as np
import pytest

from conftest import bits_equal
from ac_measure_host import pyacmeasure as pam
from spicey_amd import abi
from spicey_amd.ac_measure import reduce_ac_reference


@pytest.fixture(scope="module")
def cases():
    """(n_freq, n_v) -> (out_v, out_i, pool, reference rows), computed once."""
    out = {}
    for nf in pam.N_FREQS:
        for nv in pam.N_VS:
            v, i = pam.buffers(nf, nv, seed=1000 * nf + nv)
            pool = pam.request_pool(nf, nv, pam.N_I, seed=nf + nv)
            out[(nf, nv)] = (v, i, pool, reduce_ac_reference(v, i, pool))
    return out


def test_pool_covers_every_option(cases):
    v, i, pool, ref = cases[(300, 5)]
    assert len(pool) >= 200
    cr = pool[pool["kind"] == abi.AC_MEAS_CROSS]
    for field, vals in (("what", (0, 1, 2)), ("dir", (-1, 0, 1)), ("which", (0, 1)), ("rel", (0, 1))):
        assert set(cr[field].tolist()) == set(vals), field
    assert set(pool["what"].tolist()) == {0, 1, 2} and set(pool["num_signal"].tolist()) == {0, 1} and set(pool["den_signal"].tolist()) == {-1, 0, 1}
    assert (pool["num_col_ref"] >= 0).any() and (pool["den_col_ref"] >= 0).any() and (pool["k_from"] == pool["k_to"]).any()
    assert ((pool["k_from"] > 0) & (pool["k_to"] > pool["k_from"])).any()
    # the planted samples are seen: crossings with more than one hit, NaN rows
    assert (ref[:, pool["kind"] == 1, 0] > 1).any() and np.isnan(ref).any()


@pytest.mark.parametrize("nf", pam.N_FREQS)
@pytest.mark.parametrize("nv", pam.N_VS)
def test_harness_equals_reference_bit_for_bit(cases, nf, nv):
    v, i, pool, ref = cases[(nf, nv)]
    got = pam.run(v, i, pool)
    bad = ~bits_equal(got, ref)
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], ref[bad][:5])


@pytest.mark.parametrize("lanes,waves", [(1, 0), (2, 5), (16, 1), (64, 7)])
def test_launch_geometry_does_not_matter(cases, lanes, waves):
    for key in ((65, 2), (300, 5)):
        v, i, pool, ref = cases[key]
        assert bits_equal(pam.run(v, i, pool, lanes=lanes, waves=waves), ref).all()


def test_first_occurrence_nan_and_zero_denominator(cases):
    v, i, pool, ref = cases[(129, 2)]
    nf = 129
    ext = pam.make_ac_reqs([(0, 0, -1, -1, 0, 0, abi.AC_WHAT_MAG2, abi.AC_MEAS_EXTREMA, 0, -1, 0.0, 0, 0, 0),   # plateau of instance 2
                            (1, 1, -1, -1, 0, 0, abi.AC_WHAT_RE, abi.AC_MEAS_EXTREMA, 0, -1, 0.0, 0, 0, 0),     # NaN first sample (instance 2)
                            (0, 0, -1, 0, 1, -1, abi.AC_WHAT_MAG2, abi.AC_MEAS_EXTREMA, nf // 3, nf // 3, 0.0, 0, 0, 0),  # / the zero sample
                            (0, 0, -1, 0, 1, -1, abi.AC_WHAT_MAG2, abi.AC_MEAS_EXTREMA, 0, -1, 0.0, 0, 0, 0)])
    got = pam.run(v, i, ext)
    assert bits_equal(got, reduce_ac_reference(v, i, ext)).all()
    assert got[2, 0, 1] == 3.125 and got[2, 0, 3] == nf // 4                   # the plateau's FIRST sample is the maximum
    assert np.isnan(got[2, 1, :2]).all() and (got[2, 1, 2:4] == 0).all()     # m = NaN stays, at k_from
    assert not np.isnan(got[1, 0, :2]).any() and got[1, 0, 2] != nf // 2     # a NaN in the middle never becomes an extreme
    assert np.isnan(got[0, 2, [0, 1, 4, 5]]).all() and got[0, 2, 2] == nf // 3  # x / 0 = (0 / 0, 0 / 0): the IEEE result, no throw
    assert not np.isnan(got[0, 3]).any()                                     # and over the whole sweep it is never an extreme


def test_subsets_and_single_requests_give_the_same_rows(cases):
    v, i, pool, ref = cases[(300, 5)]
    rng = np.random.default_rng(5)
    pick = rng.permutation(len(pool))[:60]
    assert bits_equal(pam.run(v, i, pool[pick]), ref[:, pick]).all()
    for r in pick[:12]:
        assert bits_equal(pam.run(v, i, pool[r:r + 1]), ref[:, r:r + 1]).all()
    assert bits_equal(pam.run(v[1:2], i[1:2], pool), ref[1:2]).all()  # and n_inst does not matter


def test_refusals():
    nf, nv = 65, 2
    v, i = pam.buffers(nf, nv, seed=3)
    good, bad = pam.refusals(nf, nv, pam.N_I)
    assert pam.run(v, i, good).shape == (pam.N_INST, 1, 8)
    for name, reqs, have_i in bad:
        with pytest.raises(pam.Refused, match="ac measure"):
            pam.run(v, i if have_i else None, reqs)
    assert pam.lib().spicey_acm_host_workspace_bytes(3, 65, 0) == -1
    assert pam.lib().spicey_acm_host_workspace_bytes(3, 65, 5) == 512  # the table alone, rounded up to 256 bytes
