"""CPU (stubbed library): dispatch of the 2-D Winograd weight gradient of the dense 3x3 convs.
With the generous stub fp32 training issues emsa_conv_wgrad_wino2d exactly once per selected dense
conv; with the plain stub (every `*_supported` query answers 0) or with the switch off it issues none
and the launches of the existing dry-run tests stay what they were."""
import torch

import test_host_logic as H
from test_host_logic import fake_lib, generous_lib  # noqa: F401  (fixtures)


def _train_step(monkeypatch):
    """one fp32 training step at 64x96 on the stub -> the ConvSpecs handed to Fn.conv_wgrad"""
    import emsanet_amd.model as M
    from emsanet_amd import full_args, functional as Fn
    from oracle.emsanet_oracle import synthetic_batch
    specs = []
    inner = Fn.conv_wgrad

    def recording(x, dy, spec, *a, **kw):
        specs.append(spec)
        return inner(x, dy, spec, *a, **kw)
    monkeypatch.setattr(Fn, 'conv_wgrad', recording)
    model = H._model(full_args(input_height=64, input_width=96)).train()
    monkeypatch.setattr(M.EMSANet, 'forward', H._bypass_device_check(model))
    outs = model(synthetic_batch(2, 64, 96))
    flat = [t for o, sides in outs for t in (list(o) if isinstance(o, tuple) else [o])]
    flat += [t for _, sides in outs for s in sides for t in (list(s) if isinstance(s, tuple) else [s])]
    torch.autograd.backward(flat, [torch.zeros_like(t) for t in flat])
    assert all(p.grad is not None and p.grad.shape == p.shape for p in model.parameters())
    monkeypatch.setattr(Fn, 'conv_wgrad', inner)
    return specs


def test_generous_stub_one_launch_per_selected_dense_conv(generous_lib, monkeypatch):
    from emsanet_amd import functional as Fn
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', None)
    monkeypatch.setattr(Fn, '_WGRAD_WINO2D_ENV', None)
    before = Fn.WGRAD_WINO2D_FALLBACKS
    specs = _train_step(monkeypatch)
    eligible = [s for s in specs if Fn.wino2d_eligible(s)]
    selected = [s for s in eligible if Fn.wgrad_wino2d_selected(s)]
    # three decoder modules in two decoders, the two heads' 3x3 convs and the merged task convs
    assert len(eligible) == 9, [(s.cin, s.cout) for s in eligible]
    assert Fn.WGRAD_WINO2D_SHAPES <= {(s.cin, s.cout) for s in eligible}
    assert len(selected) == sum((s.cin, s.cout) in Fn.WGRAD_WINO2D_SHAPES for s in eligible)
    c = generous_lib.calls
    assert c['emsa_conv_wgrad_wino2d'] == len(selected)
    assert c['emsa_conv_wgrad_wino2d_supported'] == len(selected)
    assert Fn.WGRAD_WINO2D_FALLBACKS == before


def test_generous_stub_forced_on_and_off(generous_lib, monkeypatch):
    from emsanet_amd import functional as Fn
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', True)
    specs = _train_step(monkeypatch)
    n_on = generous_lib.calls['emsa_conv_wgrad_wino2d']
    assert n_on == sum(Fn.wino2d_eligible(s) for s in specs) == 9
    row_on = generous_lib.calls['emsa_conv_wgrad']
    generous_lib.calls.clear()
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', False)
    _train_step(monkeypatch)
    c = generous_lib.calls
    assert c['emsa_conv_wgrad_wino2d'] == 0 and c['emsa_conv_wgrad_wino2d_supported'] == 0
    assert c['emsa_conv_wgrad'] == row_on + n_on         # the same convs, on the row kernel


def test_plain_stub_issues_none_and_counts_the_fallbacks(fake_lib, monkeypatch):
    from emsanet_amd import functional as Fn
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', True)
    before = Fn.WGRAD_WINO2D_FALLBACKS
    specs = _train_step(monkeypatch)
    c = fake_lib.calls
    assert c['emsa_conv_wgrad_wino2d'] == 0
    n = sum(Fn.wino2d_eligible(s) for s in specs)
    assert c['emsa_conv_wgrad_wino2d_supported'] == n == Fn.WGRAD_WINO2D_FALLBACKS - before
