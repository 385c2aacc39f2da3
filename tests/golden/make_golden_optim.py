#!/usr/bin/env python
"""Generate tests/golden/optim.npz: the reference's SharedAdam and SharedRMSprop (shared_optim.py) RUN for 8 steps on three
small tensors, so that tests/optim_spec.py and the package's optimizers can be held to them without the reference checkout.

Run once, where the reference checkout is (the GPU box never sees it):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_optim.py

Configurations: SharedAdam with amsgrad on / off x weight_decay 0 / 1e-2 (lr 1e-3, eps 1e-3: its defaults), SharedRMSprop
with weight_decay 0 / 1e-2 (lr 7e-4, alpha 0.99, eps 0.1: its defaults). The gradient of step 2 is 300x larger than the
others (beta2 = 0.999 weighs it by 1e-3, so it takes that much for the later second moments to fall): AMSGrad's maximum stays
above the running second moment for the rest of the run. Stored per configuration "<cfg>/": the
hyper-parameters, and per tensor k the initial weights w0_k, the gradients g_k [STEPS, ...], the weights p_k [STEPS, ...] and
every state tensor (exp_avg_k, exp_avg_sq_k, max_exp_avg_sq_k / square_avg_k) after each step. The output is DATA: the
reference is imported, none of its text is stored. make_golden.py is imported for its path set-up.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import numpy as np  # noqa: E402

SHAPES = ((7, 5), (1,), (13,))
STEPS, SPIKE = 8, 2
CONFIGS = [("adam_ams%d_wd%d" % (a, w > 0), "adam", dict(amsgrad=bool(a), weight_decay=w)) for a in (1, 0) for w in (0, 1e-2)]
CONFIGS += [("rmsprop_wd%d" % (w > 0), "rmsprop", dict(weight_decay=w)) for w in (0, 1e-2)]


def optim_fixture():
    import torch
    sys.path.insert(0, mg.REF)
    import shared_optim as ref
    rs = np.random.RandomState(11)
    w0 = [(rs.randn(*s) * 0.5).astype(np.float32) for s in SHAPES]
    grads = [rs.randn(STEPS, *s).astype(np.float32) * 0.1 for s in SHAPES]
    for g in grads:
        g[SPIKE] *= 300.0
        g.reshape(STEPS, -1)[4, 0] = 0.0                       # one exactly-zero gradient entry
    out = dict(shapes=np.array([str(s) for s in SHAPES]), steps=np.int64(STEPS), spike=np.int64(SPIKE),
               configs=np.array([c[0] for c in CONFIGS]))
    for name, kind, kw in CONFIGS:
        params = [torch.nn.Parameter(torch.from_numpy(w.copy())) for w in w0]
        opt = ref.SharedAdam(params, **kw) if kind == "adam" else ref.SharedRMSprop(params, **kw)
        state_names = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if kind == "adam" else ("square_avg",)
        rec = {"p": [[] for _ in SHAPES]}
        rec.update({s: [[] for _ in SHAPES] for s in state_names})
        for t in range(STEPS):
            for k, p in enumerate(params):
                p.grad = torch.from_numpy(grads[k][t].copy())
            opt.step()
            for k, p in enumerate(params):
                rec["p"][k].append(p.detach().numpy().copy())
                for s in state_names:
                    rec[s][k].append(opt.state[p][s].numpy().copy())
        g0 = opt.param_groups[0]
        pre = name + "/"
        out[pre + "kind"] = np.array(kind)
        for key in ("lr", "eps", "weight_decay") + (("alpha",) if kind == "rmsprop" else ()):
            out[pre + key] = np.float64(g0[key])
        if kind == "adam":
            out[pre + "betas"] = np.array(g0["betas"], np.float64)
            out[pre + "amsgrad"] = np.bool_(g0["amsgrad"])
        for k in range(len(SHAPES)):
            out[pre + "w0_%d" % k] = w0[k]
            out[pre + "g_%d" % k] = grads[k]
            for key, v in rec.items():
                out[pre + "%s_%d" % (key, k)] = np.stack(v[k])
        print(name, "final |p| sums", [float(np.abs(rec["p"][k][-1]).sum()) for k in range(len(SHAPES))])
    np.savez_compressed(os.path.join(HERE, "optim.npz"), **out)


if __name__ == "__main__":
    optim_fixture()
