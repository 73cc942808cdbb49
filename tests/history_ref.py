"""NumPy restatement of the history record (include/hakai_hip.h, hakai_history_enable).

Works from per-step arrays: the state before a step (disp = u_k, disp_pre = u_{k-1}), the Q and
external force that step's nodal update consumes, and the displacement after it (u_{k+1}). Every
value is the exactly rounded sum (math.fsum) of its per-dof terms; next to it comes the sum of the
terms' magnitudes, which scales the error bound of a floating-point summation of the same terms.

Terms, per dof d of a node of the set (m its mass, du = u_{k+1} - u_k, dup = u_k - u_{k-1},
v = du / dt, ck = (du + dup) / 2):
    F_int Q        F_ext f        P m v        KE 1/2 m v^2        U u_k
    W_int Q ck     W_ext f ck
    W_bc  at prescribed dofs the three products m (du - dup) / dt^2 ck, Q ck and -f ck (the
          constraint force's three parts, so the magnitudes do not cancel)
"""
import math

import numpy as np

FIELDS = ("F_int_x", "F_int_y", "F_int_z", "F_ext_x", "F_ext_y", "F_ext_z", "P_x", "P_y", "P_z", "KE", "W_int",
          "W_ext", "W_bc", "U_x", "U_y", "U_z")
NF = 16
U = 2.0 ** -53


def fsum(a):
    return math.fsum(np.asarray(a, np.float64).ravel().tolist())


def prescribed_mask(model):
    """Per dof: some *Boundary entry of the model prescribes it."""
    p = np.zeros(3 * model.nNode, bool)
    for g in model.bc:
        for dofs, _ in g.entries:
            p[np.asarray(dofs, np.int64) - 1] = True
    return p


class HistoryRef:
    def __init__(self, diag_M, prescribed, sets, dt):
        """diag_M: 3nN lumped mass per dof; prescribed: 3nN bool; sets: the caller's sets (1-based
        node ids), set 0 = every node is added in front."""
        self.m = np.asarray(diag_M, np.float64)
        self.nN = self.m.size // 3
        self.presc = np.asarray(prescribed, bool)
        self.sets = [np.arange(self.nN)] + [np.asarray(s, np.int64).ravel() - 1 for s in sets]
        self.dt = float(dt)
        self.du_prev = None
        self.ke_seed = None
        self.work_steps = None  # [set][3]: the per-step work sums so far

    def _dofs(self, s):
        n = self.sets[s]
        return (3 * n[:, None] + np.arange(3)[None, :])  # (nodes, 3)

    def seed(self, disp, disp_pre):
        """(Re)start: du_prev, zero works; returns (KE_seed, sum |term|) per set."""
        self.du_prev = np.asarray(disp) - np.asarray(disp_pre)
        v = self.du_prev / self.dt
        ke = 0.5 * self.m * v * v
        S = len(self.sets)
        self.work_steps = [[[] for _ in range(3)] for _ in range(S)]
        self.ke_seed = np.array([fsum(ke[self._dofs(s)]) for s in range(S)])
        return self.ke_seed, np.array([fsum(np.abs(ke[self._dofs(s)])) for s in range(S)])

    def step(self, disp_new, disp, Q, fext=None):
        """One step's record: (values (sets, 16), magnitudes (sets, 16)); the works are the totals
        since the seed, their magnitudes this step's alone."""
        m, dt = self.m, self.dt
        disp_new, disp, Q = (np.asarray(a, np.float64) for a in (disp_new, disp, Q))
        f = np.zeros_like(disp) if fext is None else np.asarray(fext, np.float64)
        du = disp_new - disp
        dup = self.du_prev
        v = du / dt
        ck = 0.5 * (du + dup)
        P = m * v
        ke = 0.5 * m * v * v
        wi = Q * ck
        we = f * ck
        pr = self.presc
        wb = np.stack([np.where(pr, m * (du - dup) / (dt * dt) * ck, 0.0), np.where(pr, Q * ck, 0.0),
                       np.where(pr, -(f * ck), 0.0)], axis=-1)  # (3nN, 3)
        S = len(self.sets)
        val, mag = np.zeros((S, NF)), np.zeros((S, NF))
        for s in range(S):
            d = self._dofs(s)
            for c in range(3):
                for base, arr in ((0, Q), (3, f), (6, P), (13, disp)):
                    val[s, base + c] = fsum(arr[d[:, c]])
                    mag[s, base + c] = fsum(np.abs(arr[d[:, c]]))
            val[s, 9], mag[s, 9] = fsum(ke[d]), fsum(np.abs(ke[d]))
            for j, arr in enumerate((wi[d], we[d], wb[d])):
                self.work_steps[s][j].append(fsum(arr))
                val[s, 10 + j] = math.fsum(self.work_steps[s][j])
                mag[s, 10 + j] = fsum(np.abs(arr))
        self.du_prev = du
        return val, mag


def balance(val, ke_seed):
    """KE - KE_seed + W_int - W_ext - W_bc of one set's values, and the largest of its terms."""
    terms = [val[9], -ke_seed, val[10], -val[11], -val[12]]
    return math.fsum(terms), max(abs(t) for t in terms)
