"""The first evaluation of the leave-one-out objective on a fresh handle.  The tail's vectors are allocated and cleared by that
first call; the clearing runs on the handle's stream, in front of the tail's kernels.  (Cleared on the null stream it could land
behind them -- the handle's streams do not wait for the null stream -- and the first evaluation returned L_LOO = 0 with a zero
gradient, all later ones the right numbers.)  So: the first evaluation has the second's bits and lies inside the project's bounds
of the references, on several fresh handles and under both objectives of option 49."""
import numpy as np
import pytest

import loo_ref as ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", [4, 9])
def test_the_first_evaluation_of_a_fresh_handle_is_the_second(i):
    from andvaranaut_amd import MiGP

    X, y, kernel, theta, diag, cond = ref.case(i)
    v_ref, (_, g_ref), _ = ref.case_refs(i)
    for block in (1, 1, 1, 10):
        gp = MiGP(X, y, kernel, device=0)
        if diag is not None:
            gp.set_diag(diag)
        first = gp.cv_grad(theta, block) if block > 1 else gp.loo_grad(theta)
        again = gp.cv_grad(theta, block) if block > 1 else gp.loo_grad(theta)
        gp.close()
        assert first[0] == again[0] and np.array_equal(first[1], again[1]) and first[1].any(), (block, first, again)
        if block == 1:
            assert ref.value_ratio(first[0], v_ref, cond) <= 1.0 and ref.grad_ratio(first[1], g_ref, cond) <= 1.0
