"""A differentiable solve for torch: u = solve(solver, f, alpha, beta_i, beta_j, beta_k) with gradients to f and to the coefficients
(DESIGN.md §11.9).

    s = Solver(n, bc="dirichlet", a=0.0, b=1.0)
    u = solve(s, f, None, beta_i, beta_j, beta_k, boundary=g)     # GPU float64 tensors; beta_* with requires_grad
    loss = ((u - u_obs) ** 2).sum()
    loss.backward()                                                # beta_i.grad, beta_j.grad, beta_k.grad

Forward: set_coefficients on the detached tensors, then Solver.solve.  Backward: the operator is symmetric, so the adjoint is one more solve,
lam = solve(grad_u) with the same method and rtol and NO boundary data; then G = Solver.sensitivity(u, lam, boundary=g) in one pass, and the
gradients are lam for f and -G for alpha and the betas.  `boundary` and `robin` are not differentiable.

solve_cells(solver, f, alpha, k, mean="harmonic") is the same for a cell-centred conductivity k (one (N,N,N) tensor): forward
set_cell_coefficients, backward Solver.cell_sensitivity(u, lam, k), the gradients lam, -d_alpha and -d_k.

Backward leaves lam as the solver's "last solution" (get_solution()) and its right-hand side as grad_u.  The gradient is accurate to about the
larger of the two solves' rtol.  The solver's coefficients must be the forward's when backward runs: a set_coefficients, set_shift or march
between the two raises.  torch is imported inside the functions: the package imports without it.
"""


def _function(cells):
    """The autograd.Function of solve (cells False: coefficients alpha, beta_i, beta_j, beta_k) or of solve_cells (True: alpha, k and, before them, the
    mean): one body, which differs in the set_ call of forward and the sensitivity call of backward."""
    import torch

    class _Solve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, boundary, robin, method, rtol, max_iter, mean, f, *coef):
            coef = [None if c is None else c.detach().contiguous() for c in coef]
            if cells:
                solver.set_cell_coefficients(*coef, mean=mean, robin=robin)
            else:
                solver.set_coefficients(*coef, robin=robin)
            u, info = solver.solve(f.detach().contiguous(), method=method, rtol=rtol, boundary=boundary, max_iter=max_iter)
            if not info.converged:
                raise RuntimeError(f"solve: the forward solve did not converge (residual {info.residual:.3e}, |f| {info.norm_f:.3e}, rtol {rtol:g})")
            ctx.solver, ctx.boundary, ctx.method, ctx.rtol, ctx.max_iter, ctx.mean = solver, boundary, method, rtol, max_iter, mean
            ctx.version = solver.coefficient_version
            ctx.save_for_backward(u, *([coef[1]] if cells else []))
            return u

        @staticmethod
        def backward(ctx, grad_u):
            solver = ctx.solver
            u = ctx.saved_tensors[0]
            if solver.coefficient_version != ctx.version:
                raise RuntimeError("solve: the solver's coefficients changed between forward and backward (set_coefficients, set_shift or a march)")
            lam, info = solver.solve(grad_u.contiguous(), method=ctx.method, rtol=ctx.rtol, max_iter=ctx.max_iter)
            if not info.converged:
                raise RuntimeError(f"solve: the adjoint solve did not converge (residual {info.residual:.3e}, |grad_u| {info.norm_f:.3e}, rtol {ctx.rtol:g})")
            if cells:
                G = solver.cell_sensitivity(u, lam, ctx.saved_tensors[1], mean=ctx.mean, boundary=ctx.boundary)
            else:
                G = solver.sensitivity(u, lam, boundary=ctx.boundary)
            need = ctx.needs_input_grad[7:]
            grads = [lam if need[0] else None] + [-g if (g is not None and want) else None for g, want in zip(G, need[1:])]
            return (None,) * 7 + tuple(grads)

    return _Solve


_cached = {}


def _apply(cells, solver, boundary, robin, method, rtol, max_iter, mean, *arrays):
    for name, x in (("boundary", boundary), ("robin", robin)):
        if getattr(x, "requires_grad", False):
            raise ValueError(f"{name}: not differentiable (detach it; only f and the coefficients carry gradients)")
    if cells not in _cached:
        _cached[cells] = _function(cells)
    return _cached[cells].apply(solver, boundary, robin, method, rtol, max_iter, mean, *arrays)


def solve(solver, f, alpha, beta_i, beta_j, beta_k, boundary=None, robin=None, method="mg", rtol=1e-10, max_iter=100):
    """u with A u = f + T(boundary) for the coefficients given, differentiable in f, alpha and the betas (module docstring).  All arrays are GPU
    float64 tensors as Solver takes them; alpha is None on a Poisson solver.  Raises ValueError if `boundary` or `robin` requires grad, and
    RuntimeError if a solve reports converged == False or the solver's coefficients changed before backward."""
    return _apply(False, solver, boundary, robin, method, rtol, max_iter, None, f, alpha, beta_i, beta_j, beta_k)


def solve_cells(solver, f, alpha, k, mean="harmonic", boundary=None, robin=None, method="mg", rtol=1e-10, max_iter=100):
    """solve for a cell-centred conductivity k (N,N,N) in place of the three face arrays (Solver.set_cell_coefficients),
    differentiable in f, alpha and k: forward is set_cell_coefficients and solve, backward lam = solve(grad_u) and Solver.cell_sensitivity(u, lam, k),
    and the gradients are lam, -d_alpha and -d_k.  Raises what solve raises."""
    return _apply(True, solver, boundary, robin, method, rtol, max_iter, mean, f, alpha, k)
