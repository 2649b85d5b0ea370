"""Float64 restatement of the batched 2-D exact k-space propagator (include/kwave_hip.h "Exact k-space propagator on
frames"; a plain module, imported by name from tests/): tests/second_order_reference.py with expanded = (Ex, Ey, 1), whose kz
is 0 on its single plane, frame by frame.  Arrays are [F][y][x]; n, d and expanded are given as (x, y).

    p_f(t) = irfft2( rfft2(p0_f embedded in Ey x Ex) H(|k|; t) ),  |k|^2 = kx^2 + ky^2
"""
import numpy as np

import second_order_reference as sr

rel_l2, neper, default_sides = sr.rel_l2, sr.neper, sr.default_sides


def plane(expanded):
    return (expanded[0], expanded[1], 1)


def spacings(d):
    return (d[0], d[1], 1.0)   # the third spacing multiplies kz = 0


def H(expanded, d, c0, t, alpha_coeff=0.0, y=1.5):
    """[Ey][Ex/2 + 1]"""
    return sr.H(plane(expanded), spacings(d), c0, t, alpha_coeff, y)[0]


def b_margins(expanded, d, c0, alpha_coeff, y):
    return sr.b_margins(plane(expanded), spacings(d), c0, alpha_coeff, y)


def stage_case(expanded):
    """sr.stage_case on the plane: spacings sr.STAGE_D[:2]"""
    return sr.stage_case(plane(expanded))


def solve_expanded(vol, d, c0, t, alpha_coeff=0.0, y=1.5):
    """every expanded plane of vol [F][Ey][Ex] at time t"""
    return np.array([sr.solve_expanded(v[None], spacings(d), c0, t, alpha_coeff, y)[0] for v in np.asarray(vol, dtype=np.float64)])


def solve(p0, expanded, d, c0, times, alpha_coeff=0.0, y=1.5):
    """[n_times][F][Ny][Nx]: the domain crop of every frame at every time"""
    out = [sr.solve(f[None], plane(expanded), spacings(d), c0, times, alpha_coeff, y)[:, 0] for f in np.asarray(p0, dtype=np.float64)]
    return np.stack(out, axis=1)
