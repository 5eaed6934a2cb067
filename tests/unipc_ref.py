"""fp64 reference of the UniPC multistep sampler behind the reference's ``FlowAdapterScheduler`` (flow_adapter.py with its default
``base_scheduler='UniPCMultistep'``): diffusers' ``UniPCMultistepScheduler`` with ``prediction_type='flow_prediction'``,
``use_flow_sigmas=True``, ``predict_x0=True``, ``lower_order_final=True``, ``final_sigmas_type='zero'`` -- as recalled; diffusers is not a
dependency of this project and nothing pins this arithmetic against it.

Written in the loop form of the scheduler itself on purpose: a list of past x0-predictions, per-k ``r_k`` and ``D_k``, the ``R`` / ``b``
system and a ``solve``.  ``arcflow_amd.schedule.FlowUniPCScheduler.coefficients`` flattens the same update into one weight per operand; the
tests hold the two against each other, so nothing here may use the flattened form.
"""
import numpy as np


def lam(s):
    """lambda(s) = log(1 - s) - log s (alpha = 1 - s for flow sigmas); +inf at s = 0."""
    with np.errstate(divide='ignore'):
        return np.log1p(-s) - np.log(s)


def _system(order, rks, hh, bh2):
    """-> (R, b, h phi_1, B) of one update, hh = -h."""
    h_phi_1 = np.expm1(hh)
    B = np.expm1(hh) if bh2 else hh
    h_phi_k = h_phi_1 / hh - 1.0
    R, b, f = [], [], 1.0
    for j in range(1, order + 1):
        R.append(np.power(rks, j - 1))
        b.append(h_phi_k * f / B)
        f *= j + 1
        h_phi_k = h_phi_k / hh - 1.0 / f
    return np.stack(R), np.array(b), h_phi_1, B


def sample(model, x, sigmas, base_sigmas, solver_order=2, solver_type='bh2', begin=0, trajectory=False):
    """Roll ``x`` (fp64 array) over steps begin .. n - 1 of the schedule.  sigmas [n + 1] (trailing 0): what the model is evaluated at, as
    the adapter hands its own timesteps to the denoiser; base_sigmas [n + 1] = sigmas clamped to 1 - eps: what the solver computes with.
    model(x, sigma, i) -> the velocity u.  The history is empty at ``begin``.  trajectory: also return every step's result."""
    sg = np.asarray(base_sigmas, dtype=np.float64)
    st = np.asarray(sigmas, dtype=np.float64)
    n = len(sg) - 1
    bh2 = {'bh1': False, 'bh2': True}[solver_type]
    outs, last, lower, this_order, traj = [], None, 0, None, []
    x = np.asarray(x, dtype=np.float64)
    for i in range(begin, n):
        u = model(x, st[i], i)
        m_t = x - sg[i] * u                                   # convert_model_output: x0 = sample - sigma * flow, from the uncorrected sample
        if i > begin:                                         # multistep_uni_c_bh_update at order this_order of the previous step
            s_t, s_0, o = sg[i], sg[i - 1], this_order
            h = lam(s_t) - lam(s_0)
            m0 = outs[-1]
            rks, D1s = [], []
            for k in range(1, o):
                rk = (lam(sg[i - (k + 1)]) - lam(s_0)) / h
                rks.append(rk)
                D1s.append((outs[-(k + 1)] - m0) / rk)
            rks.append(1.0)
            R, b, h_phi_1, B = _system(o, np.array(rks), -h, bh2)
            rhos_c = np.array([0.5]) if o == 1 else np.linalg.solve(R, b)
            x_t_ = s_t / s_0 * last - (1.0 - s_t) * h_phi_1 * m0
            corr_res = sum(r * d for r, d in zip(rhos_c[:-1], D1s)) if D1s else 0.0
            D1_t = m_t - m0
            x = x_t_ - (1.0 - s_t) * B * (corr_res + rhos_c[-1] * D1_t)
        outs.append(m_t)
        outs = outs[-solver_order:]
        this_order = min(min(solver_order, n - i), lower + 1)       # lower_order_final, then the warm-up
        last = x
        s_t, s_0, o = sg[i + 1], sg[i], this_order                  # multistep_uni_p_bh_update
        m0 = outs[-1]
        if s_t == 0.0:                                              # h = +inf: expm1(-inf) = -1; the order is 1 here, no D terms
            assert o == 1
            x = s_t / s_0 * x - (1.0 - s_t) * (-1.0) * m0
        else:
            h = lam(s_t) - lam(s_0)
            rks, D1s = [], []
            for k in range(1, o):
                rk = (lam(sg[i - k]) - lam(s_0)) / h
                rks.append(rk)
                D1s.append((outs[-(k + 1)] - m0) / rk)
            rks.append(1.0)
            R, b, h_phi_1, B = _system(o, np.array(rks), -h, bh2)
            x_t_ = s_t / s_0 * x - (1.0 - s_t) * h_phi_1 * m0
            if D1s:
                rhos_p = np.array([0.5]) if o == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
                x = x_t_ - (1.0 - s_t) * B * sum(r * d for r, d in zip(rhos_p, D1s))
            else:
                x = x_t_
        if lower < solver_order:
            lower += 1
        traj.append(x)
    return (x, traj) if trajectory else x


def euler(model, x, sigmas):
    """The first-order ODE sampler on the same schedule (FlowEulerODEScheduler in fp64)."""
    st = np.asarray(sigmas, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    for i in range(len(st) - 1):
        x = x + model(x, st[i], i) * (st[i + 1] - st[i])
    return x

