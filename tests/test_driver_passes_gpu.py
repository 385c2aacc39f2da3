"""The elementwise / gather / scatter launches of csrc/driver_hip.hip that cap their grid, each just above its cap.

Their other direct tests stay below the caps, so a grid-stride trip, a row split or a chunk loop that went wrong would show
only as one term of an 800 000-element norm in a whole-learner test:
  * atr_relu_backward_ld and atr_embed_add_ld launch at most 4096 workgroups = 1 048 576 float4 per pass;
  * atr_embed_grad gives each workgroup 64 rows up to 65 536 rows and splits the rows over 1024 workgroups beyond, and keeps
    kEmbMaxA = 8 accumulators per column of which the tests so far used 4;
  * FlatParams.set_grads hands atr_scatter_segments at most 64 segments per launch.

Tolerances: exact equality (relu backward, set_grads, repeat calls); for embed_add one ulp of the output plus one ulp of
w + b around the float64 value (the kernel rounds w + b, then the sum: half an ulp each, and the float64 value may sit in the
binade below the rounded one); for embed_grad tests/f64_rule.Table.rule against float64 sums with x32 = the one-hot matmul
in fp32 through PyTorch.

Measured on MI355X: embed_add's worst error / (ulp(out) + ulp(w + b)) is 0.500 in all seven cases; embed_grad at 81 920 rows
has e(hip) 1.2e-7 .. 1.6e-7 against e(aten32) 2.5e-7 .. 9.3e-7 for dw, its columns and db with 4 and 8 actions (the kernel's
fixed two-level order beats the matmul's); everything else is exact equality.
"""
import pytest
import torch

import f64_rule
import optim_spec as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.25


def test_relu_backward_above_the_grid_cap():
    """1 049 600 float4 (cap: 1 048 576), dense and read from a 384-wide store: equal to aten's threshold_backward."""
    from active_tracking_rl_amd import fused
    torch.manual_seed(0)
    for rows, C, ld in ((4100, 1024, 1024), (16400, 256, 384)):
        assert rows * C // 4 == 1049600
        store = torch.randn(rows, ld, device=DEV)
        f = store[:, :C]
        df = torch.randn(rows, C, device=DEV)
        got = fused.relu_backward_ld(df, f)
        want = torch.ops.aten.threshold_backward(df, f.contiguous(), 0.0)
        assert torch.equal(got, want), (rows, C, ld, int((got != want).sum()))
        assert 0.4 < float((want == 0).float().mean()) < 0.6


def _action_store(rows, A, gen_seed):
    """Actions of one player as the [T, N] view of a [T, 2, N] store (T N = rows) the learner reads them from; the other
    player's column holds a different action everywhere."""
    T = next(t for t in (4, 3, 2, 1) if rows % t == 0)
    N = rows // T
    g = torch.Generator().manual_seed(gen_seed)
    store = torch.randint(0, A, (T, 2, N), generator=g).to(DEV)
    store[:, 0] = (store[:, 1] + 1) % A
    return store, store[:, 1]


EMBED_ADD_CASES = [(r, 256, A) for r in (16383, 16384, 16400) for A in (4, 8)] + [(8200, 512, 8)]


@pytest.mark.parametrize("rows,C,A", EMBED_ADD_CASES)
def test_embed_add_around_the_grid_cap(rows, C, A):
    """out = f + (w[:, a] + b) per row at 1 048 512 / 1 048 576 / 1 049 600 float4 (and A C = kEmbTabMax = 4096 floats of
    LDS table), features read from a wider store, actions in place from a [T, 2, N] store: every element within
    ulp32(out) + ulp32(w + b) of float64, and the same bits from a dense copy of the features and a flat copy of the actions."""
    from active_tracking_rl_amd import fused
    torch.manual_seed(rows + A)
    lin = torch.nn.Linear(A, C).to(DEV)
    with torch.no_grad():
        lin.weight.mul_(3.0)
    store = torch.randn(rows, C + 128, device=DEV)
    f = store[:, :C]
    _, acts = _action_store(rows, A, rows)
    flat = acts.reshape(-1)
    assert len(torch.unique(flat)) == A
    with torch.no_grad():
        out = fused.embed_add(f, lin, acts)
        again = fused.embed_add(f.contiguous(), lin, flat.clone())
    assert torch.equal(out, again)
    e64 = (lin.weight.detach().double().t() + lin.bias.detach().double())[flat]            # [rows, C]
    want = f.double() + e64
    tol = S.ulp32(want.cpu()) + S.ulp32(e64.cpu())
    err = (out.double() - want).abs().cpu()
    worst = float((err / tol).max())
    print("embed_add rows %d C %d A %d: worst error / (ulp(out) + ulp(w + b)) = %.3f" % (rows, C, A, worst))
    assert worst <= 1.0, (worst, int((err / tol).argmax()) // C)


EMBED_GRAD_ROWS = [1, 63, 64, 65, 4097, 65535, 65536, 65537, 81920]


@pytest.mark.parametrize("A", [4, 8])
@pytest.mark.parametrize("rows", EMBED_GRAD_ROWS)
def test_embed_grad_across_the_row_split(rows, A):
    """dw[c][a] = sum of dout[r][c] over the rows with action a, db[c] = sum over all rows, at one row, around one workgroup's
    64 rows, and around / above the 65 536 rows where the split changes, with 4 and 8 actions: against float64 sums under
    Table.rule (x32 = one-hot matmul in fp32 through PyTorch); a second call gives the same bits."""
    from active_tracking_rl_amd import fused
    C = 256
    torch.manual_seed(rows * 8 + A)
    lin = torch.nn.Linear(A, C).to(DEV)
    f = torch.randn(rows, C, device=DEV, requires_grad=True)
    _, acts = _action_store(rows, A, rows + 1)
    dout = torch.randn(rows, C, device=DEV) * (1.0 + torch.arange(C, device=DEV) % 7)
    out = fused.embed_add(f, lin, acts)
    df, dw, db = torch.autograd.grad(out, [f, lin.weight, lin.bias], dout, retain_graph=True)
    _, dw2, db2 = torch.autograd.grad(out, [f, lin.weight, lin.bias], dout)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(df, dout)
    assert dw.shape == (C, A) and db.shape == (C,)
    onehot = torch.nn.functional.one_hot(acts.reshape(-1), A)
    dw64 = dout.double().t() @ onehot.double()
    dw32 = dout.t() @ onehot.float()
    table = f64_rule.Table("embed_grad rows %d A %d" % (rows, A))
    table.rule("dw", dw, dw64, dw32)
    for a in range(A):                                   # per action too: one dropped accumulator is 1 / A of the norm at most
        table.rule("dw[:, %d]" % a, dw[:, a], dw64[:, a], dw32[:, a])
    table.rule("db", db, dout.double().sum(0), dout.sum(0))
    table.finish()


LENGTHS = (1, 3, 1023, 1024, 1025, 4097)


def test_set_grads_on_the_device_in_three_launches():
    """150 parameters = 64 + 64 + 22 segments. Sources: odd-offset slices of one packed buffer, a non-contiguous tensor, a
    float64 tensor, None (the slot becomes zero), and slices already in place (left alone), over a bucket pre-filled with a
    sentinel: the slots are bit-equal to a CPU FlatParams fed the same gradients, the padding keeps the sentinel."""
    from active_tracking_rl_amd.shared_optim import FlatParams
    gen = torch.Generator().manual_seed(4)
    shapes = [(LENGTHS[(i * 5 + i // 6) % 6],) for i in range(150)]
    shapes[7], shapes[20], shapes[72], shapes[140] = (31, 33), (33, 31), (31, 33), (5, 205)   # 1023 / 1025 elements, 2-d
    assert {s[0] for s in shapes if len(s) == 1} == set(LENGTHS)
    cpu_params = [torch.nn.Parameter(torch.zeros(*s)) for s in shapes]
    gpu_params = [torch.nn.Parameter(torch.zeros(*s, device=DEV)) for s in shapes]
    cb, gb = FlatParams(cpu_params), FlatParams(gpu_params)
    offsets, total = S.layout(shapes)
    assert gb.offsets == offsets == cb.offsets and gb.numel == total
    gb.grad.fill_(SENTINEL)
    views = gb.grad_views()
    packed_cpu = torch.randn(sum(p.numel() for p in cpu_params) + 151, generator=gen)
    packed = packed_cpu.to(DEV)
    cpu_grads, gpu_grads, pos, kinds = [], [], 1, {}
    for i, s in enumerate(shapes):
        n = cpu_params[i].numel()
        kind = ("none" if i % 11 == 3 else "in_place" if i % 13 == 5 else "noncontig" if len(s) == 2 else
                "float64" if i % 7 == 2 else "packed")
        kinds[kind] = kinds.get(kind, 0) + 1
        src = packed_cpu[pos:pos + n].reshape(s)
        if kind == "none":
            cpu_grads.append(None); gpu_grads.append(None)
        elif kind == "in_place":
            views[i].copy_(src)
            cpu_grads.append(src.clone()); gpu_grads.append(views[i])
        elif kind == "noncontig":
            t = src.t().contiguous().to(DEV).t()
            assert not t.is_contiguous() and t.shape == s
            cpu_grads.append(src.clone()); gpu_grads.append(t)
        elif kind == "float64":
            cpu_grads.append(src.clone()); gpu_grads.append(src.double().to(DEV))
        else:
            g = packed[pos:pos + n].view(s)
            assert pos % 2 == 1 and g.data_ptr() % 8 == 4
            cpu_grads.append(src.clone()); gpu_grads.append(g)
        pos += n + n % 2                                             # (every slice starts at an odd float)
    assert min(kinds.get(k, 0) for k in ("none", "in_place", "noncontig", "float64", "packed")) >= 3
    assert {i // 64 for i in range(150) if i % 11 == 3} == {0, 1, 2}               # a None in every launch
    cb.set_grads(cpu_grads)
    gb.set_grads(gpu_grads)
    torch.cuda.synchronize()
    got = gb.grad.cpu()
    pad = torch.ones(total, dtype=torch.bool)
    for i, (off, p) in enumerate(zip(offsets, cpu_params)):
        n = p.numel()
        pad[off:off + n] = False
        assert torch.equal(got[off:off + n], cb.grad[off:off + n]), (i, shapes[i])
        assert gpu_params[i].grad.data_ptr() == gb.grad.data_ptr() + 4 * off
        if cpu_grads[i] is None:
            assert float(got[off:off + n].abs().max()) == 0.0
    assert int(pad.sum()) > 100 and bool((got[pad] == SENTINEL).all())
    assert float(cb.grad[pad].abs().max()) == 0.0
