#!/usr/bin/env python
"""Generate tests/golden/model_gru.npz: make_golden.py::model_fixture for the GRU nets ("tat-maze-gru", "maze-gru").

Run once, where the reference checkout is (the GPU box never sees it):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_gru.py

The reference A3C_Dueling.forward(test=True) (model.py:238-265, GRU branches :120-124, :139-141, :169-173, :198-200) is RUN on the
deterministic weights of make_golden.det_weights and the same 6 samples (RandomState(5), drawn in the same order, so states / hx /
cx equal model.npz's) under the same key names. The output is DATA (inputs + expected outputs): the reference is imported, none
of its text is stored. make_golden.py is imported for its path set-up (tests/golden/_refstubs) and det_weights.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts _refstubs and the reference env package on sys.path)
import numpy as np  # noqa: E402

NETS = ("tat-maze-gru", "maze-gru")


def model_fixture_gru():
    import torch
    sys.path.insert(0, mg.REF)
    import model as ref_model
    from gym import spaces
    out = {}
    rs = np.random.RandomState(5)
    for net in NETS:
        args = argparse.Namespace(stack_frames=1, rnn_out=128, network=net, single=False)
        obs_space = [spaces.Box(0, 6, (1, 13, 13), np.float32) for _ in range(2)]
        act_space = [spaces.Discrete(4) for _ in range(2)]
        torch.manual_seed(0)
        m = ref_model.build_model(obs_space, act_space, args, torch.device("cpu"))
        sd = m.state_dict()
        keys = sorted(sd.keys())
        p = net + "/"
        for k, name in enumerate(keys):
            sd[name].copy_(torch.from_numpy(mg.det_weights(tuple(sd[name].shape), k)))
        m.eval()
        B = 6
        states = rs.choice([0, 1, 2, 4], size=(B, 2, 1, 1, 13, 13)).astype(np.float32)
        hx = rs.randn(B, 2, 128).astype(np.float32) * 0.3
        cx = rs.randn(B, 2, 128).astype(np.float32) * 0.3
        vals, acts, ents, lps, hxo, cxo, rp = [], [], [], [], [], [], []
        for b in range(B):
            with torch.no_grad():
                v, a, e, lp, (h, c), r = m((torch.from_numpy(states[b]), (torch.from_numpy(hx[b]), torch.from_numpy(cx[b]))), True)
            vals.append(v.numpy()); acts.append([int(x) for x in a]); ents.append(e.numpy()); lps.append(lp.numpy())
            hxo.append(h.numpy()); cxo.append(c.numpy())
            rp.append(np.asarray(r.numpy() if hasattr(r, "numpy") else r, np.float32).reshape(-1))
        out[p + "keys"] = np.array(keys); out[p + "shapes"] = np.array([str(tuple(sd[k].shape)) for k in keys])
        out[p + "states"] = states; out[p + "hx"] = hx; out[p + "cx"] = cx
        out[p + "values"] = np.array(vals); out[p + "actions"] = np.array(acts); out[p + "entropies"] = np.array(ents)
        out[p + "log_probs"] = np.array(lps); out[p + "hx_out"] = np.array(hxo); out[p + "cx_out"] = np.array(cxo)
        out[p + "r_pred"] = np.array(rp)
        out[p + "n_params"] = np.int64(sum(v.numel() for v in sd.values()))
        print(net, "params", int(out[p + "n_params"]), "values", np.array(vals).shape)
    np.savez_compressed(os.path.join(HERE, "model_gru.npz"), **out)


if __name__ == "__main__":
    model_fixture_gru()
