"""Batched damped-least-squares position IK on the GPU Jacobian.

Restates ``dls_ik_position_only`` (ctr_reach_envs/src/jacobian_controller.py:19-73) for a batch
of targets: every iteration takes the forward-difference Jacobian J and the tip P of the env's
forward kinematics (CtrReachVecEnv.jacobian, one ctr_jacobian launch for the whole batch), then

    e  = P_d - P
    q += J^T (J J^T + lam I)^-1 e
    stop (per target) once |e| < tol          (checked after the update, as the reference does)

The reference builds a CTR_Model (its BVP model) for J; here J is the env's own FK
(model.py:30-70), so the IK is consistent with the environment the policy acts in.  Plotting
is omitted.  A target whose iterate leaves the nesting constraints into a tube gap (NaN FK; the
reference's solver loops forever there) stops at its last finite iterate with err = NaN.

``fused=True`` runs the same loop in one kernel launch (CtrReachVecEnv.ik_dls, ctr_ik_dls: a wave
owns its targets from q0 to the stop, no per-iteration launches and no host reads), and
dls_ik_path follows waypoint paths (the reference's line / circle / helix paths in src/) with it:
waypoint k starts from waypoint k - 1's solution.
"""
from ._abi import CTR_IK_MAX_ITERS


def dls_ik_position_only(env, targets, q0, system=None, lam=0.25, num=500, tol=1e-3, eps=1e-4, check_every=8,
                         fused=False):
    """targets [M, 3], q0 [M, 6] (float64 tensors or arrays) -> (q [M, 6], err [M], iters [M]).

    ``fused=True``: the whole loop in one ctr_ik_dls launch (``check_every`` then has no meaning;
    num <= CTR_IK_MAX_ITERS).  The default is the stream-ordered loop below.

    The iteration is stream-ordered: every iteration runs on the whole batch with finished targets
    masked out, and the host reads the "any target still active" flag only every
    ``check_every`` iterations (to stop early), so the loop does not synchronise per iteration."""
    import torch
    dev = env.device
    if fused:
        pd = torch.as_tensor(targets, dtype=torch.float64, device=dev).reshape(-1, 3)
        return env.ik_dls(pd, q0, system=system, lam=lam, num=num, tol=tol, eps=eps)[:3]
    pd = torch.as_tensor(targets, dtype=torch.float64, device=dev).reshape(-1, 3)
    q = torch.as_tensor(q0, dtype=torch.float64, device=dev).reshape(-1, 6).clone()
    m = q.shape[0]
    sys_t = None if system is None else torch.as_tensor(system, dtype=torch.int32, device=dev).reshape(-1).expand(m)
    active = torch.ones(m, dtype=torch.bool, device=dev)
    err = torch.full((m,), float("inf"), dtype=torch.float64, device=dev)
    iters = torch.zeros(m, dtype=torch.int32, device=dev)
    eye = lam * torch.eye(3, dtype=torch.float64, device=dev)
    nan = torch.tensor(float("nan"), dtype=torch.float64, device=dev)
    for k in range(int(num)):
        if k % max(1, int(check_every)) == 0 and not bool(active.any()):
            break
        p, jac = env.jacobian(q, sys_t, eps=eps)
        e = pd - p
        # an iterate that left the nesting constraints into a tube gap (NaN FK, where the
        # reference's solver never returns) stops at its last finite iterate with err = NaN
        bad = active & (~torch.isfinite(e).all(dim=1) | ~torch.isfinite(jac).flatten(1).all(dim=1))
        err = torch.where(bad, nan, err)
        live = active & ~bad
        jl = torch.where(live[:, None, None], jac, torch.zeros_like(jac))
        el = torch.where(live[:, None], e, torch.zeros_like(e))
        jjt = jl @ jl.transpose(1, 2) + eye
        dq = (jl.transpose(1, 2) @ torch.linalg.solve(jjt, el.unsqueeze(-1))).squeeze(-1)
        q = torch.where(live[:, None], q + dq, q)
        en = torch.linalg.norm(el, dim=1)
        err = torch.where(live, en, err)
        iters = iters + live.to(torch.int32)
        active = live & (en >= tol)
    return q, err, iters


def dls_ik_path(env, waypoints, q0, system=None, lam=0.25, num=500, tol=1e-3, eps=1e-4,
                max_iters_per_launch=CTR_IK_MAX_ITERS):
    """Follow a waypoint path: waypoints [M, K, 3], q0 [M, 6] -> (q [M, K, 6], err [M, K],
    iters [M, K]), the DLS IK of every waypoint started from the previous waypoint's solution
    (q0 for the first), each with at most ``num`` iterations.

    The path is cut into ctr_ik_dls launches at waypoint boundaries, floor(max_iters_per_launch /
    num) waypoints each; a launch starts from the last waypoint's q of the one before.  The
    launches are stream-ordered: the host reads nothing between them."""
    import torch
    dev = env.device
    wp = torch.as_tensor(waypoints, dtype=torch.float64, device=dev)
    if wp.dim() != 3 or wp.shape[-1] != 3 or wp.shape[1] < 1:
        raise ValueError("waypoints must be [M, K, 3] with K >= 1")
    num, cap = int(num), min(int(max_iters_per_launch), CTR_IK_MAX_ITERS)
    if num > cap:
        raise ValueError("num = %d exceeds max_iters_per_launch = %d" % (num, cap))
    k = wp.shape[1]
    per = k if num == 0 else max(1, min(k, cap // num))
    q = torch.as_tensor(q0, dtype=torch.float64, device=dev).reshape(-1, 6)
    qs, errs, its = [], [], []
    for k0 in range(0, k, per):
        qk, ek, ik, _ = env.ik_dls(wp[:, k0:k0 + per], q, system=system, lam=lam, num=num, tol=tol, eps=eps)
        q = qk[:, -1].contiguous()
        qs.append(qk)
        errs.append(ek)
        its.append(ik)
    if len(qs) == 1:
        return qs[0], errs[0], its[0]
    return torch.cat(qs, dim=1), torch.cat(errs, dim=1), torch.cat(its, dim=1)
