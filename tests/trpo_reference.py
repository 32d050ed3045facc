"""The reference's TRPO policy step restated in torch f64 on the CPU (src/algorithms/trpo.py:14-84,
345-424) for test_trpo_host.py and test_gpu_trpo.py: mu by F.linear / activation, the KL with the
epsilon on the new variance, the double-backward Hessian-vector product, conjugate gradient and
the backtracking line search.  Nothing here goes through mepol_amd.policy's custom Functions or
mepol_amd.algorithms.trpo."""
import math

import torch
import torch.nn.functional as F


class RefPolicy:
    """Plain tensors: Ws / bs of the hidden layers, Wm, bm, log_std; `act` the activation.
    params() is in the order of GaussianPolicy.parameters(): log_std, the hidden layers' weight
    and bias in turn, then the mean layer's."""

    def __init__(self, Ws, bs, Wm, bm, log_std, act=torch.relu):
        cp = lambda t: t.detach().to("cpu", torch.float64).clone().requires_grad_(True)
        self.Ws, self.bs = [cp(W) for W in Ws], [cp(b) for b in bs]
        self.Wm, self.bm, self.log_std = cp(Wm), cp(bm), cp(log_std)
        self.act = act

    @classmethod
    def from_policy(cls, policy, act=torch.relu):
        import torch.nn as nn

        layers = [m for m in policy.net if isinstance(m, nn.Linear)]
        return cls([m.weight for m in layers], [m.bias for m in layers], policy.mean.weight,
                   policy.mean.bias, policy.log_std, act)

    @classmethod
    def random(cls, nf, hidden, a, seed, act=torch.relu, log_std=-0.5):
        g = torch.Generator().manual_seed(seed)
        widths = [nf] + list(hidden)
        Ws = [torch.randn(o, i, generator=g, dtype=torch.float64) * math.sqrt(2.0 / i)
              for i, o in zip(widths[:-1], widths[1:])]
        bs = [0.1 * torch.randn(o, generator=g, dtype=torch.float64) for o in widths[1:]]
        Wm = torch.randn(a, widths[-1], generator=g, dtype=torch.float64) / math.sqrt(widths[-1])
        bm = 0.1 * torch.randn(a, generator=g, dtype=torch.float64)
        ls = log_std + 0.2 * torch.randn(a, generator=g, dtype=torch.float64)
        return cls(Ws, bs, Wm, bm, ls, act)

    def params(self):
        out = [self.log_std]
        for W, b in zip(self.Ws, self.bs):
            out += [W, b]
        return out + [self.Wm, self.bm]

    def flat(self):
        return torch.cat([p.detach().reshape(-1) for p in self.params()])

    def assign(self, flat):
        o = 0
        with torch.no_grad():
            for p in self.params():
                p.copy_(flat[o:o + p.numel()].view(p.shape))
                o += p.numel()

    def load_into(self, policy):
        """Copies these parameters into a GaussianPolicy of the same shape."""
        with torch.no_grad():
            for p, q in zip(policy.parameters(), self.params()):
                assert p.shape == q.shape
                p.copy_(q.to(p.device))

    def mean(self, x):
        h = x
        for W, b in zip(self.Ws, self.bs):
            h = self.act(F.linear(h, W, b))
        return F.linear(h, self.Wm, self.bm)

    def log_p(self, x, actions):
        mu = self.mean(x)
        std = torch.exp(self.log_std) + 1e-7
        return torch.sum(-0.5 * (math.log(2 * math.pi) + 2 * self.log_std
                                 + (actions - mu) ** 2 / std ** 2), dim=1)


def kl(mu0, log_std0, mu1, log_std1):
    var0 = torch.exp(log_std0) ** 2
    var1 = torch.exp(log_std1) ** 2
    return (0.5 * ((var0 + (mu1 - mu0) ** 2) / (var1 + 1e-7) - 1)
            + log_std1 - log_std0).sum(dim=1).mean()


def make_hvp(ref, x, damping):
    """hessian_vector_product of the reference at ref's current parameters over states x."""
    mu0 = ref.mean(x).detach()
    ls0 = ref.log_std.detach().clone()

    def hvp(v):
        k = kl(mu0, ls0, ref.mean(x), ref.log_std)
        grads = torch.autograd.grad(k, ref.params(), create_graph=True)
        flat = torch.cat([g.reshape(-1) for g in grads])
        grads2 = torch.autograd.grad(torch.sum(flat * v), ref.params())
        return torch.cat([g.reshape(-1) for g in grads2]) + damping * v

    return hvp


def conj_gradient(Ax, b, iters):
    x = torch.zeros_like(b)
    r = b.clone()
    p = r.clone()
    i = 0
    while True:
        Ap = Ax(p)
        rr = torch.dot(r, r)
        alpha = rr / torch.dot(p, Ap)
        x = x + alpha * p
        i += 1
        if i == iters:
            break
        r_new = r - alpha * Ap
        beta = torch.dot(r_new, r_new) / rr
        p = r_new + beta * p
        r = r_new
    return x


def trpo_step(ref, x, actions, adv, kl_thresh, cg_iters=10, damping=0.1, max_iters=10):
    """The reference's policy update on ref (in place).  Returns (success, backtrack_iters,
    trials, x_dir) with trials = [(improvement, kl)] of every backtracking trial made."""
    old_lp = ref.log_p(x, actions).detach()
    mu0 = ref.mean(x).detach()
    ls0 = ref.log_std.detach().clone()

    def gain():
        return torch.mean(torch.exp(ref.log_p(x, actions) - old_lp) * adv)

    hvp = make_hvp(ref, x, damping)
    g = torch.cat([t.reshape(-1) for t in torch.autograd.grad(gain(), ref.params())])
    xdir = conj_gradient(hvp, g, cg_iters)
    lagrange = torch.sqrt(torch.dot(xdir, hvp(xdir)) / (2 * kl_thresh))
    old = ref.flat()
    old_obj = gain().item()
    trials = []
    for i in range(max_iters):
        ref.assign(old + 0.5 ** i * (1 / lagrange) * xdir)
        with torch.no_grad():
            imp = gain().item() - old_obj
            k = kl(mu0, ls0, ref.mean(x), ref.log_std).item()
        trials.append((imp, k))
        if math.isfinite(imp) and imp > 0 and math.isfinite(k) and k < kl_thresh:
            return True, i, trials, xdir
    ref.assign(old)
    return False, max_iters - 1, trials, xdir


def closed_form_hvp(ref, x, v, damping):
    """The closed form of DESIGN.md, "TRPO policy step", in plain torch (ReLU networks)."""
    with torch.no_grad():
        n = x.shape[0]
        L = len(ref.Ws)
        o = 0
        vs = []
        for p in ref.params():
            vs.append(v[o:o + p.numel()].view(p.shape))
            o += p.numel()
        v_ls, v_net, v_Wm, v_bm = vs[0], vs[1:1 + 2 * L], vs[-2], vs[-1]
        hs, masks = [x], []
        for W, b in zip(ref.Ws, ref.bs):
            h = torch.relu(F.linear(hs[-1], W, b))
            masks.append((h > 0).to(x.dtype))
            hs.append(h)
        t = torch.zeros_like(x)
        for l in range(L):
            t = masks[l] * (t @ ref.Ws[l].t() + hs[l] @ v_net[2 * l].t() + v_net[2 * l + 1])
        u = torch.exp(2 * ref.log_std)
        c = (t @ ref.Wm.t() + hs[L] @ v_Wm.t() + v_bm) / ((u + 1e-7) * n)
        out = [None] * (2 * L)
        dWm, dbm = c.t() @ hs[L], c.sum(0)
        dz = (c @ ref.Wm) * masks[L - 1]
        for l in range(L - 1, -1, -1):
            out[2 * l], out[2 * l + 1] = dz.t() @ hs[l], dz.sum(0)
            if l:
                dz = (dz @ ref.Ws[l]) * masks[l - 1]
        d_ls = 2 * u * u * (u - 1e-7) / (u + 1e-7) ** 3 * v_ls
        flat = torch.cat([t.reshape(-1) for t in [d_ls] + out + [dWm, dbm]])
        return flat + damping * v


def per_tensor_rel(ref_params, got, want):
    """Largest over the parameter tensors of max |got - want| / max |want|."""
    worst, o = 0.0, 0
    for p in ref_params:
        k = p.numel()
        g, w = got[o:o + k], want[o:o + k]
        worst = max(worst, (g - w).abs().max().item() / max(w.abs().max().item(), 1e-300))
        o += k
    return worst
