"""Prescribed rigid-body motion for the time-step drivers (`NotebookSimulation(..., motion=...)`): pistons, paddles,
stirrers, shaken tanks.  Host side, numpy / scipy; the only device traffic is two small uploads per step (the moved
bodies' rows of `rb_d` and the angular velocities `rb_w` that `sdf.evaluate_grid` reads).

A `Motion` is a linear and an angular velocity, each a constant or a function of time.  `BodyKinematics` integrates them:
the schedule is sampled at the step's start and held over the step (the solid velocity the pressure solve and the boundary
condition see is then the one the body really moved with), T += v dt, R <- Rot(w dt) R about the body's own centre.
"""
import numpy as np
import torch
from scipy.spatial.transform import Rotation


class Motion:
    """velocity: D-vector; omega: 3-vector (rad/s) in 3D, scalar in 2D.  Either may be a callable of the time t."""

    def __init__(self, velocity=None, omega=None):
        self.velocity, self.omega = velocity, omega

    @staticmethod
    def _at(value, t, shape):
        if value is None:
            return np.zeros(shape)
        if callable(value):
            value = value(t)
        return np.broadcast_to(np.asarray(value, np.float64), shape).copy()

    def velocity_at(self, t, dim):
        return self._at(self.velocity, t, (dim,))

    def omega_at(self, t, dim):
        return self._at(self.omega, t, (3,) if dim == 3 else ())


class BodyKinematics:
    """rb_d: the packed bodies of solver.sdf3D (n, 10, 4) / solver.sdf2D (n, 8, 3), updated IN PLACE by `advance`;
    motion: {body index: Motion}; dim: 3 or 2.  Poses of the moving bodies are mirrored on the host in float64, the
    rotation as a scipy `Rotation` (3D) or an angle (2D), so that it stays orthonormal over any number of steps.
    `rb_w`: float64 (n, 3) / (n,) on rb_d's device, the angular velocities of the current step (0 for bodies at rest)."""

    def __init__(self, rb_d, motion, dim):
        if dim not in (2, 3):
            raise ValueError(f"dim: 2 or 3, got {dim}")
        shape = (10, 4) if dim == 3 else (8, 3)
        if not isinstance(rb_d, torch.Tensor) or rb_d.dim() != 3 or tuple(rb_d.shape[1:]) != shape or rb_d.dtype != torch.float64:
            raise ValueError(f"rb_d: expected a float64 tensor of shape (n, {shape[0]}, {shape[1]})")
        n = int(rb_d.shape[0])
        self.rb_d, self.dim, self.motion = rb_d, dim, {int(i): m for i, m in motion.items()}
        for i, m in self.motion.items():
            if not 0 <= i < n:
                raise ValueError(f"motion: no body {i} among {n}")
            if not isinstance(m, Motion):
                raise TypeError(f"motion[{i}]: expected a Motion, got {type(m).__name__}")
        self.indices = sorted(self.motion)
        self._idx = torch.as_tensor(self.indices, dtype=torch.int64, device=rb_d.device)
        host = rb_d.detach().cpu().numpy()
        self._rows = host[self.indices].copy()                    # (m,) + shape: what is uploaded, row 0 never changes
        D = dim
        self.T = {i: host[i, 1:1 + D, D].copy() for i in self.indices}
        if D == 3:
            self.R = {i: Rotation.from_matrix(host[i, 5:8, :3]) for i in self.indices}
        else:
            self.R = {i: float(np.arctan2(host[i, 5, 0], host[i, 4, 0])) for i in self.indices}
        self.rho = {i: float(np.linalg.norm(host[i, 0, 1:])) for i in self.indices}
        self.rb_w = torch.zeros((n, 3) if D == 3 else (n,), dtype=torch.float64, device=rb_d.device)

    def rotation_matrix(self, i):
        """(D, D) float64 rotation of moving body i"""
        if self.dim == 3:
            return self.R[i].as_matrix()
        c, s = np.cos(self.R[i]), np.sin(self.R[i])
        return np.array(((c, -s), (s, c)))

    def max_surface_speed(self, t):
        """bound on the speed of any surface point of any moving body at time t: |v| + |w| rho, rho the norm of the
        body's row-0 parameters (>= its extent from the centre for a sphere, a box and a cylinder)"""
        out = 0.0
        for i in self.indices:
            m = self.motion[i]
            out = max(out, float(np.linalg.norm(m.velocity_at(t, self.dim)) + np.linalg.norm(m.omega_at(t, self.dim)) * self.rho[i]))
        return out

    def advance(self, t, dt):
        """move every body by its velocities at time t held over dt; rb_d rows and rb_w follow"""
        if not self.indices:
            return
        D = self.dim
        w_all = np.zeros((len(self.indices),) + ((3,) if D == 3 else ()))
        for k, i in enumerate(self.indices):
            m = self.motion[i]
            v, w = m.velocity_at(t, D), m.omega_at(t, D)
            self.T[i] = self.T[i] + v * dt
            if D == 3:
                self.R[i] = Rotation.from_rotvec(w * dt) * self.R[i]
            else:
                self.R[i] = self.R[i] + float(w) * dt
            rows = self._rows[k]
            rows[1:1 + D, D] = self.T[i]                      # translation rows: the identity with T in the last column
            rows[1 + D + 1:1 + D + 1 + D, :D] = self.rotation_matrix(i)
            rows[-1, :D] = v
            w_all[k] = w
        dev = self.rb_d.device
        self.rb_d[self._idx, 1:] = torch.as_tensor(self._rows[:, 1:], device=dev)
        self.rb_w[self._idx] = torch.as_tensor(w_all, device=dev)
