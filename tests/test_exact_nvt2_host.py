"""The restatement the exact NVT2 mode relies on, on the CPU (no device): the reference's second normal vote is the
same function as its first (Processor.py:110-117: getBetterFilteredNVT on the filtered normals), so the host builds
of the kernels' vote + tensor sums (`pcd_host_nvt_tensor`: normalised by Σw) and of the LAPACK ssyevd restatement
(`pcd_host_eigh3`) on the second vote's inputs -- `pos0`, `it1_f_n`, the fixture's kNN lists, rho = 5π/12 -- must give
the reference's `it1_eigval2` / `it1_eigvec2` bit for bit, and the classes of those eigenvalues `it1_classes`.
k_nvt2_exact (csrc/denoise.hip) runs these two functions' device builds."""
import math

import numpy as np
import pytest

import pcd_native as nat
from oracle import pcd_oracle as O

RHO = math.pi * 5 / 12


@pytest.mark.parametrize("k", [32, 16])
def test_host_second_vote_is_the_reference_bitwise(golden, k):
    f = golden(f"fandisk_k{k}")
    pos0, fn, knn = f["pos0"], f["it1_f_n"], f[f"knn{k}"].astype(np.int64)
    N = len(pos0)
    t6 = nat.host_nvt_tensor(pos0, fn, np.arange(N), np.arange(N + 1) * k, knn.reshape(-1), RHO)
    w, V = nat.host_eigh3(t6)
    np.testing.assert_array_equal(w, f["it1_eigval2"])
    np.testing.assert_array_equal(V, f["it1_eigvec2"])
    np.testing.assert_array_equal(O.classes(w), f["it1_classes"])
