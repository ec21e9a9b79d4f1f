"""Full-batch L-BFGS for the K softmax regressions of csrc/logreg.hip, minimised as ONE problem.

The objectives F_p (include/itcv_hip.h) are separable -- problem p owns the columns ``coff[p]:coff[p + 1]`` of
``theta[(D + 1), csum]`` -- so their sum is minimised over the stacked parameters: memory 10, backtracking Armijo line
search, start at zero.  One value/gradient launch per evaluation; ``x``, ``y`` and the parameters stay on the device and
a handful of scalars (the values, g.d, max|grad| per problem, the two error flags) is read back once per evaluation.

The stopping rule is part of the contract: ``max|grad F_p| <= gtol`` for EVERY problem p.  If ``max_iter`` iterations
do not reach it, ``RuntimeError`` names the worst problem; an unconverged result is never returned.
"""
import torch

__all__ = ["minimize", "LBFGS_MEMORY"]

LBFGS_MEMORY = 10
ARMIJO_C1 = 1e-4
FLAT_EPS = 1e-14


def _segment_absmax(g, bounds):
    """max|g| over each problem's columns: a [K] tensor (bounds: python ints, the prefix sums of the class counts)."""
    colmax = g.abs().amax(dim=0)
    return torch.stack([colmax[a:b].max() for a, b in zip(bounds[:-1], bounds[1:])])


def minimize(valgrad, shape, bounds, device, gtol=1e-9, max_iter=2000, check=None):
    """Minimise ``sum_p F_p``.  ``valgrad(theta) -> (f[K], grad)`` (fp64 device tensors); ``bounds``: the K + 1 column
    offsets of the problems; ``check``: an optional pair (tensor getter, handler) whose
    values ride along with every read-back (the kernels' error flags).
    Returns ``(theta, info)`` with ``info = {"iterations", "evaluations", "f": [K floats], "gmax": [K floats]}``."""
    K = len(bounds) - 1
    theta = torch.zeros(shape, dtype=torch.float64, device=device)
    evals = 0

    def evaluate(t, d=None):
        """One launch, one read-back: (sum f, g.d, [f_p], [max|g_p|], grad)."""
        nonlocal evals
        evals += 1
        f, g = valgrad(t)
        gd = (g * d).sum().reshape(1) if d is not None else f.new_zeros(1)
        parts = [f, _segment_absmax(g, bounds), gd]
        if check is not None:
            parts.append(check[0]().to(torch.float64))
        host = torch.cat(parts).tolist()
        if check is not None:
            check[1](host[2 * K + 1:])
        return sum(host[:K]), host[2 * K], host[:K], host[K:2 * K], g

    fsum, _, fp, gmax, g = evaluate(theta)
    S, Y, RHO = [], [], []
    it = 0
    while max(gmax) > gtol:
        if it >= max_iter:
            worst = max(range(K), key=lambda p: gmax[p])
            raise RuntimeError(f"logreg: L-BFGS did not reach max|grad| <= {gtol:g} within {max_iter} iterations: "
                               f"problem {worst} is at {gmax[worst]:.3e}")
        it += 1
        # two-loop recursion
        q = g.clone()
        alphas = []
        for s, yv, rho in zip(reversed(S), reversed(Y), reversed(RHO)):
            a = rho * (s * q).sum()
            q.sub_(a * yv)
            alphas.append(a)
        if S:
            q.mul_((S[-1] * Y[-1]).sum() / (Y[-1] * Y[-1]).sum())
        else:
            q.mul_(1.0 / max(1.0, float(g.abs().sum())))
        for (s, yv, rho), a in zip(zip(S, Y, RHO), reversed(alphas)):
            b = rho * (yv * q).sum()
            q.add_((a - b) * s)
        d = q.neg_()
        gd0 = float((g * d).sum())
        if not gd0 < 0.0:                                   # not a descent direction: restart from steepest descent
            S, Y, RHO = [], [], []
            d = g.neg()
            gd0 = float((g * d).sum())
        step, ok = 1.0, False
        for _ in range(60):
            cand = theta + step * d
            fs2, gd2, fp2, gmax2, g2 = evaluate(cand, d)
            if fs2 <= fsum + ARMIJO_C1 * step * gd0:
                ok = True
                break
            # Near the optimum the decrease of f drops below its rounding error (f - f* ~ |grad|^2 / (2 lambda)) long before
            # max|grad| reaches gtol.  There the slope decides (the approximate Wolfe condition of Hager and Zhang):
            # f is unchanged to rounding and the directional derivative has shrunk without overshooting.
            if fs2 <= fsum + FLAT_EPS * abs(fsum) and (2.0 * ARMIJO_C1 - 1.0) * gd0 >= gd2 >= 0.9 * gd0:
                ok = True
                break
            step *= 0.5
        if not ok:
            if S:                                           # rounding has eaten the model: drop it and try the gradient
                S, Y, RHO = [], [], []
                continue
            worst = max(range(K), key=lambda p: gmax[p])
            raise RuntimeError(f"logreg: the line search found no decrease; problem {worst} is at max|grad| = "
                               f"{gmax[worst]:.3e} (gtol {gtol:g})")
        s, yv = cand - theta, g2 - g
        sy = float((s * yv).sum())
        if sy > 1e-300:
            S.append(s), Y.append(yv), RHO.append(1.0 / sy)
            if len(S) > LBFGS_MEMORY:
                S.pop(0), Y.pop(0), RHO.pop(0)
        theta, fsum, fp, gmax, g = cand, fs2, fp2, gmax2, g2
    return theta, {"iterations": it, "evaluations": evals, "f": fp, "gmax": gmax}
