"""The device's summary-statistics chain (hydra_ss_chain on hgibbs_ss_sweep) with a band that covers every pair
against the CPU oracle's individual-level chain: the cases and the comparison rule of tests/test_ss_host_vs_oracle_cpu.py.  The band
is the device's own, built from the loaded image with hgibbs_ld's products (W = M - 1); b = X'y comes from NumPy's standardised
columns, as in the CPU test."""
import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c[0] for c in sc.CASES])
def test_device_chain_is_the_oracles_chain(oracle, name):
    ref, bed, X, band, b, kw = sc.oracle_case(oracle, name)
    M, N = sc.CASE_M, sc.CASE_N
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    ch = capi.SsChain(dev, N, M - 1, b, **kw)
    # the device's band is NumPy's X'X to rounding (exact integer sums against a float matrix product)
    assert sc.close(dev.ss_band(), band, 1e-9)
    sc.assert_chain_matches_oracle(ch, ref, X)
    assert dev.last_ss_ms()[1] > 0.0
