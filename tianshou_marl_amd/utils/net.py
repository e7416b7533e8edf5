"""Actor / critic networks of the path as ONE flat HBM parameter vector.

Mirrors the reference's network stack for discrete-action PPO:
  Net(state_shape, hidden_sizes=[H, H]) -> DiscreteActor(softmax_output=False) / DiscreteCritic
  (/root/reference/tianshou/utils/net/common.py:90-181,246-369; discrete.py:27-124) joined by
  ActorCritic (common.py:461-474) so that one optimizer sees actor + critic parameters.
The fused kernels (csrc/mlp_fused.hip) read the parameters as a single flat f32 vector in
ActorCritic.parameters() order; per-layer tensors are views into it, so `state_dict()` can be
exchanged with the reference (`to_reference_state_dict`).
"""
from __future__ import annotations

import functools
import inspect
import math
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from .. import ops
from ..data.batch import Batch


def ref_layer_keys(n_layers: int, scheme: str) -> list[tuple[str, str]]:
    """[(weight key, bias key)] per layer of a `FlatMLP` under the names the reference's modules give its parameters:
      "body"  a `Net(hidden_sizes=[...])` used whole: `model.model.{2 i}` (Linear, activation, Linear, ...)
      "head"  such a `Net` under a DiscreteActor / DiscreteCritic: `preprocess.model.model.{2 i}`, the output `last.model.0`
      "fc"    the CTDE nets (ctde.py:362-364, 398-400): `fc{i + 1}`
      "seq"   a bare `nn.Sequential` of Linear and activation: `{2 i}`"""
    stems = {"body": [f"model.model.{2 * i}" for i in range(n_layers)],
             "head": [f"preprocess.model.model.{2 * i}" for i in range(n_layers - 1)] + ["last.model.0"],
             "fc": [f"fc{i + 1}" for i in range(n_layers)], "seq": [str(2 * i) for i in range(n_layers)]}[scheme]
    return [(s + ".weight", s + ".bias") for s in stems]


def _generator(seed: int | None) -> torch.Generator | None:
    """A private generator at `seed` (None: the global one draws)."""
    return torch.Generator().manual_seed(seed) if seed is not None else None


def _uniform(shape, bound: float, gen: torch.Generator | None) -> torch.Tensor:
    """torch nn.Linear's draw, uniform in +-bound.  `_GroupedLayers.reset` spells its draw otherwise and the two give different
    bits for one seed: a call site stays on the one it has."""
    return torch.empty(shape).uniform_(-bound, bound, generator=gen)


class FlatNet(nn.Module):
    """A network whose parameters are ONE flat f32 vector `flat` with views over it.  A subclass states its layout once, as
    `reference_named_views(flat)`; the storage claim, twins, the optimizer's split and the checkpoints under the reference's
    names follow from that here, as do the two checks every backward starts with."""

    # False: `FlatAdam.state_dict` lists the vector as ONE parameter, not split by `reference_named_views`.  The optimizer
    # checkpoints of these nets have always had that form, and stay readable
    split_optimizer_state = True
    _saved = None   # what the last `forward(save=True)` kept for `backward`

    def __init_subclass__(cls, **kwargs) -> None:
        """Every constructor records its arguments, device, seed and storage apart, on the instance -- the outermost call
        alone, so a subclass's arguments and not those it hands up: what `clone_over` rebuilds the net from."""
        super().__init_subclass__(**kwargs)
        init = cls.__dict__.get("__init__")
        if init is None:
            return
        sig = inspect.signature(init)

        @functools.wraps(init)
        def recording(self, *args, **kw) -> None:
            if "_ctor_args" not in self.__dict__:
                given = list(sig.bind(self, *args, **kw).arguments.items())[1:]
                self.__dict__["_ctor_args"] = {k: v for k, v in given if k not in ("device", "seed", "storage")}
            init(self, *args, **kw)

        cls.__init__ = recording

    # ---- storage and twins ------------------------------------------------------------------------------------------------
    def _claim(self, n: int, storage: torch.Tensor | None, device) -> torch.Tensor:
        """Set `flat` to `n` zeros on `device`, or to `storage`: a contiguous f32 vector of n elements, possibly a slice of a
        larger joint vector (actor and critic under one optimizer).  -> the vector."""
        if storage is None:
            storage = torch.zeros(n, dtype=torch.float32, device=device)
        elif storage.numel() != n or storage.dtype != torch.float32 or not storage.is_contiguous():
            raise ValueError(f"{type(self).__name__}: storage must be a contiguous f32 vector of {n} elements")
        self.flat = nn.Parameter(storage, requires_grad=False)
        return storage

    @torch.no_grad()
    def rebind(self, storage: torch.Tensor) -> None:
        """Move the parameters into `storage` (a slice of a joint vector) and view them there.  A net with sub-nets over
        slices of its vector moves those itself (`QMIXMixer`)."""
        storage.copy_(self.flat.data)
        self.flat = nn.Parameter(storage, requires_grad=False)

    def clone_over(self, storage: torch.Tensor):
        """A net of the same class and shape viewing `storage`, which holds the init of a private generator (the actor-critic
        nets: what it held) until the caller copies over it (`lagged_copy`)."""
        return type(self)(**self._ctor_args, device=storage.device, seed=0, storage=storage)

    def sync_image(self) -> None:
        """Re-derive what the net keeps beside `flat` in another layout (call after modifying `flat` outside the optimizer):
        `DiscreteActorCritic`'s padded image.  Most nets keep nothing."""
        return None

    # ---- ONE statement of the parameters ----------------------------------------------------------------------------------
    def _vector(self, flat: torch.Tensor | None) -> torch.Tensor:
        return self.flat.data if flat is None else flat

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """[(key, view)] of `flat` (None: the net's own vector; else any vector of its layout: a gradient, an Adam moment)
        under the reference module's parameter names and shapes, in its `state_dict()` order."""
        raise NotImplementedError

    def param_views(self, flat: torch.Tensor | None = None) -> list[torch.Tensor]:
        """The parameters in the ORDER OF THE VECTOR: what `FlatAdam` splits its moments by."""
        if not self.split_optimizer_state:
            return [self._vector(flat)]
        return [v for _, v in self.reference_named_views(flat)]

    def param_shapes(self) -> list[tuple[int, ...]]:
        """The shapes `FlatAdam.state_dict` lists for this net."""
        return [tuple(v.shape) for v in self.param_views()]

    def to_reference_state_dict(self, prefix: str = "", sd: OrderedDict | None = None) -> OrderedDict:
        """Host copies of the parameters under prefix + the reference's keys, added to `sd` (None: a new OrderedDict)."""
        return export_views(self.reference_named_views(), prefix, sd)

    def load_reference_state_dict(self, sd, prefix: str = "") -> None:
        import_views(self.reference_named_views(), sd, prefix)

    # ---- what a backward starts with ----------------------------------------------------------------------------------------
    def _saved_forward(self, what: str = "backward"):
        if self._saved is None:
            raise RuntimeError(f"{type(self).__name__}.{what} called before forward")
        return self._saved

    def _slabs(self, rows: int, n_split: int, slabs: torch.Tensor | None) -> tuple[int, torch.Tensor]:
        """(n_split, slabs [n_split, n_param]) of a backward of the whole vector over `rows` rows: `n_split` <= 0 is
        `ops.mlp_n_split`'s choice, `slabs` None a fresh array."""
        P = self.flat.numel()
        if n_split <= 0:
            n_split = ops.mlp_n_split(rows)
        if slabs is None:
            slabs = torch.empty(n_split, P, dtype=torch.float32, device=self.flat.device)
        elif tuple(slabs.shape) != (n_split, P) or not slabs.is_contiguous():
            raise ValueError(f"{type(self).__name__}.backward: slabs must be a contiguous [{n_split}, {P}]")
        return n_split, slabs


def export_views(views, prefix: str = "", sd: OrderedDict | None = None) -> OrderedDict:
    """Host copies of `views` = [(key, view)] under prefix + key, added to `sd` (None: a new OrderedDict).  A view need not
    be contiguous (`BranchingNet`'s transposed branch weights); its copy is."""
    sd = OrderedDict() if sd is None else sd
    sd.update((prefix + k, v.detach().clone().contiguous().cpu()) for k, v in views)
    return sd


@torch.no_grad()
def import_views(views, sd, prefix: str = "") -> None:
    """Fill `views` = [(key, view)] from the entries of `sd` (numpy or tensors) under prefix + key."""
    for k, v in views:
        t = sd[prefix + k]
        v.copy_(torch.as_tensor(t if isinstance(t, torch.Tensor) else np.asarray(t)).to(v.device, v.dtype).reshape(v.shape))


class FlatMLP(FlatNet):
    """Fully-connected net dims[0] -> ... -> dims[-1] (hidden activation relu | tanh, linear output) whose
    parameters are ONE flat HBM vector in torch `parameters()` order; forward/backward run in csrc/dense.hip.

    `forward(x)` keeps the activations of the last call so that `backward(d_out)` can produce the gradient slabs
    (the pair replaces autograd for this module).  Layer views (`weight(i)`, `bias(i)`) alias the flat vector.
    `n_extra`: elements a subclass keeps behind the layers on the vector."""

    ref_scheme = "fc"   # of `ref_layer_keys`: the key names of `to_reference_state_dict`; any other through `export_layers`

    def __init__(self, dims, act: str = "relu", device: str | torch.device = "cuda", seed: int | None = None,
                 storage: torch.Tensor | None = None, n_extra: int = 0) -> None:
        super().__init__()
        self.dims = [int(d) for d in dims]
        self.act = act
        self.desc = ops.mlp_desc(self.dims, act)
        self.n_mlp_params = ops.mlp_param_count(self.desc)
        self._claim(self.n_mlp_params + n_extra, storage, device)
        self._offsets = []
        o = 0
        for i in range(len(self.dims) - 1):
            k, n = self.dims[i], self.dims[i + 1]
            self._offsets.append((o, o + n * k))
            o += n * k + n
        self.reset_parameters(seed)

    @property
    def n_layers(self) -> int:
        return len(self.dims) - 1

    def weight(self, i: int) -> torch.Tensor:
        o, ob = self._offsets[i]
        return self.flat.data[o:ob].view(self.dims[i + 1], self.dims[i])

    def bias(self, i: int) -> torch.Tensor:
        _, ob = self._offsets[i]
        return self.flat.data[ob:ob + self.dims[i + 1]]

    @torch.no_grad()
    def reset_parameters(self, seed: int | None = None) -> None:
        """torch nn.Linear default init (kaiming-uniform weights, uniform bias)."""
        gen = _generator(seed)
        for i, (W, b) in enumerate(self.layer_views(self.flat.data)):
            bound = 1.0 / math.sqrt(self.dims[i])
            W.copy_(_uniform(W.shape, bound, gen))
            b.copy_(_uniform(b.shape, bound, gen))

    @torch.no_grad()
    def load_layers(self, layers) -> None:
        """layers: [(W [out, in], b [out])] per layer (numpy or tensors), torch nn.Linear layout."""
        for i, (W, b) in enumerate(layers):
            self.weight(i).copy_(torch.as_tensor(np.asarray(W)).to(self.flat.device, torch.float32))
            self.bias(i).copy_(torch.as_tensor(np.asarray(b)).to(self.flat.device, torch.float32))

    def layer_views(self, flat: torch.Tensor):
        """[(W, b)] views of any flat vector with this net's layout (e.g. a summed gradient)."""
        out = []
        for i, (o, ob) in enumerate(self._offsets):
            out.append((flat[o:ob].view(self.dims[i + 1], self.dims[i]), flat[ob:ob + self.dims[i + 1]]))
        return out

    def forward(self, x: torch.Tensor, save: bool = True) -> torch.Tensor:
        x = x.to(self.flat.device, torch.float32).contiguous()
        lead = x.shape[:-1]
        if x.shape[-1] != self.dims[0]:
            raise ValueError(f"FlatMLP: input width {x.shape[-1]} != {self.dims[0]}")
        x2 = x.reshape(-1, self.dims[0])
        out, acts = ops.mlp_forward(self.desc, self.flat.data, x2)
        if save:
            self._saved = (x2, acts)
        return out.view(*lead, self.dims[-1])

    def backward(self, d_out: torch.Tensor, n_split: int = 0, slabs: torch.Tensor | None = None,
                 slab_stride: int = 0) -> torch.Tensor:
        """Gradient slabs [n_split, n_param] for the inputs of the last `forward(save=True)`; `slabs` / `slab_stride`
        direct them into the slabs of a joint parameter vector."""
        x2, acts = self._saved_forward()
        return ops.mlp_backward(self.desc, self.flat.data, x2, acts, d_out.reshape(x2.shape[0], self.dims[-1]).contiguous(),
                                n_split, slabs=slabs, slab_stride=slab_stride)

    def input_grad(self, d_out: torch.Tensor, col0: int, n_col: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient [B, n_col] w.r.t. the input columns [col0, col0 + n_col) of the last `forward(save=True)`; no weight
        gradient is computed (the critic's side of a deterministic policy gradient)."""
        x2, acts = self._saved_forward("input_grad")
        return ops.mlp_input_grad(self.desc, self.flat.data, x2, acts, d_out.reshape(x2.shape[0], self.dims[-1]), col0, n_col,
                                  out=out)

    # ---- checkpoints under the reference's key names (`ref_layer_keys`) -----------------------------------------------
    def named_layers(self, keys, prefix: str = "", flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """[(prefix + key, view)]: every layer's weight, then its bias, under `keys` = [(weight key, bias key)]; views of
        `flat` (None: the net's own vector)."""
        return [(prefix + k, v) for kk, Wb in zip(keys, self.layer_views(self._vector(flat))) for k, v in zip(kk, Wb)]

    def export_layers(self, keys, prefix: str = "", sd: OrderedDict | None = None) -> OrderedDict:
        """The layers as host copies under prefix + `keys`, added to `sd` (None: a new OrderedDict)."""
        return export_views(self.named_layers(keys), prefix, sd)

    def import_layers(self, sd, keys, prefix: str = "") -> None:
        """`load_layers` from the entries of `sd` under prefix + `keys`."""
        self.load_layers([(sd[prefix + kw], sd[prefix + kb]) for kw, kb in keys])

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        return self.named_layers(ref_layer_keys(self.n_layers, self.ref_scheme), flat=flat)


# ---- the recurrent net (utils/net/common.py:372-458) -----------------------------------------------------------------------
class Recurrent(FlatNet):
    """The reference's `Recurrent`: fc1 -> nn.LSTM(hidden, hidden, layer_num, batch_first) -> fc2 on the last step, as ONE flat
    vector in the reference's `state_dict()` order (nn.weight_ih_l0, nn.weight_hh_l0, nn.bias_ih_l0, nn.bias_hh_l0, ..., fc1.weight,
    fc1.bias, fc2.weight, fc2.bias).  The recurrence runs in csrc/lstm.hip, one launch per layer for all steps; the input
    projections, fc1, fc2 and every weight gradient on the dense engine (csrc/dense.hip).

    `forward(obs [B, L, D] | [B, D], state=None)` -> (out [B, A], state), state = (hidden, cell) in HBM as [B, layers, H];
    `state_out=(hidden, cell)` writes the new state there, and may be `state` itself: the acting step advances it in place.
    `backward(d_out)` -> gradient slabs [n_split, n_param] of sum(out * d_out) for the last `forward(save=True)`."""

    def __init__(self, *, layer_num: int, state_shape, action_shape, hidden_layer_size: int = 128,
                 device: str | torch.device = "cuda", seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        super().__init__()
        self.layer_num, self.hidden = int(layer_num), int(hidden_layer_size)
        self.obs_dim, self.n_out = int(np.prod(state_shape)), int(np.prod(action_shape))
        self.dims = [self.obs_dim, self.n_out]   # input and output width, as a FlatMLP states them
        ops.lstm_check(self.hidden, self.layer_num)
        if self.obs_dim < 1 or self.n_out < 1:
            raise ValueError(f"Recurrent: state_shape {state_shape} and action_shape {action_shape} must be non-empty")
        H = self.hidden
        shapes = [(f"nn.{p}_l{k}", sh) for k in range(self.layer_num)
                  for p, sh in (("weight_ih", (4 * H, H)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,)))]
        shapes += [("fc1.weight", (H, self.obs_dim)), ("fc1.bias", (H,)), ("fc2.weight", (self.n_out, H)), ("fc2.bias", (self.n_out,))]
        self._layout, o = [], 0
        for key, sh in shapes:
            self._layout.append((key, o, sh))
            o += math.prod(sh)
        self._off = {key: off for key, off, _ in self._layout}
        self._claim(o, storage, device)
        self.reset_parameters(seed)

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        v = self._vector(flat)
        return [(key, v[o:o + math.prod(sh)].view(sh)) for key, o, sh in self._layout]

    @torch.no_grad()
    def reset_parameters(self, seed: int | None = None) -> None:
        """torch's defaults: every nn.LSTM parameter uniform in +-1 / sqrt(hidden); nn.Linear uniform in +-1 / sqrt(fan_in)."""
        gen = _generator(seed)
        for key, v in self.reference_named_views():
            fan = self.hidden if key.startswith("nn.") or key.startswith("fc2") else self.obs_dim
            v.copy_(_uniform(v.shape, 1.0 / math.sqrt(fan), gen))

    def zero_state(self, B: int) -> tuple[torch.Tensor, torch.Tensor]:
        z = torch.zeros(2, B, self.layer_num, self.hidden, dtype=torch.float32, device=self.flat.device)
        return z[0], z[1]

    def _state(self, what: str, state, B: int):
        if state is None:
            return None
        if not isinstance(state, (tuple, list)):
            if not {"hidden", "cell"}.issubset(state.keys()):
                raise ValueError(f"Expected to find keys 'hidden' and 'cell' but instead found {state.keys()}")
            state = (state["hidden"], state["cell"])
        shape = (B, self.layer_num, self.hidden)
        out = []
        for nm, t in zip(("hidden", "cell"), state):
            t = torch.as_tensor(t)
            if what == "state":   # an input: any source, brought to the device
                t = t.to(self.flat.device, torch.float32).contiguous()
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"Recurrent: {what}.{nm} must be a contiguous device f32 {list(shape)}, got {list(t.shape)} {t.dtype}")
            out.append(t)
        return tuple(out)

    def forward(self, obs, state=None, info=None, save: bool = True, state_out=None):
        v, H, dev = self.flat.data, self.hidden, self.flat.device
        obs = torch.as_tensor(obs).to(dev, torch.float32)
        if obs.dim() == 2:
            obs = obs.unsqueeze(1)
        if obs.dim() != 3 or obs.shape[2] != self.obs_dim:
            raise ValueError(f"Recurrent: obs must be [B, L, {self.obs_dim}] or [B, {self.obs_dim}], got {list(obs.shape)}")
        obs = obs.contiguous()
        B, L = obs.shape[:2]
        ops.lstm_check(H, self.layer_num, L)
        state = self._state("state", state, B)
        hn, cn = self._state("state_out", state_out, B) if state_out is not None else self.zero_state(B)
        views = dict(self.reference_named_views())
        x = ops.dense_linear(obs.view(B * L, self.obs_dim), views["fc1.weight"], views["fc1.bias"])
        xs, layers = [], []
        for k in range(self.layer_num):
            proj = ops.dense_linear(x, views[f"nn.weight_ih_l{k}"], views[f"nn.bias_ih_l{k}"]).view(B, L, 4 * H)
            fw = ops.lstm_forward(proj, views[f"nn.weight_hh_l{k}"], views[f"nn.bias_hh_l{k}"],
                                  None if state is None else state[0][:, k], None if state is None else state[1][:, k],
                                  hn[:, k], cn[:, k], save=save)
            xs.append(x)
            layers.append(fw)
            x = fw["h"].view(B * L, H)
        out = ops.dense_linear(x.view(B, L, H)[:, L - 1], views["fc2.weight"], views["fc2.bias"])
        if save:
            self._saved = (obs, xs, layers, None if state is None else state[1])
        return out, (hn, cn)

    def backward(self, d_out: torch.Tensor, n_split: int = 0, slabs: torch.Tensor | None = None) -> torch.Tensor:
        obs, xs, layers, c0 = self._saved_forward()
        B, L = obs.shape[:2]
        H, R, off = self.hidden, B * L, self._off
        n_split, slabs = self._slabs(R, n_split, slabs)
        views = dict(self.reference_named_views())
        d_out = d_out.reshape(B, self.n_out).to(torch.float32).contiguous()
        top = layers[-1]["h"]
        ops.dense_wgrad(d_out, top[:, L - 1], slabs, n_split, off["fc2.weight"], off["fc2.bias"])
        d_h = torch.zeros(B, L, H, dtype=torch.float32, device=obs.device)   # from above: only the last step of the top layer
        ops.dense_dgrad(d_out, views["fc2.weight"], out=d_h[:, L - 1])
        for k in range(self.layer_num - 1, -1, -1):
            fw = layers[k]
            dg = ops.lstm_backward(d_h, views[f"nn.weight_hh_l{k}"], fw["gates"], fw["c"],
                                   None if c0 is None else c0[:, k])["d_gates"].view(R, 4 * H)
            ops.dense_wgrad(dg, xs[k], slabs, n_split, off[f"nn.weight_ih_l{k}"], off[f"nn.bias_ih_l{k}"])
            ops.dense_wgrad(dg, fw["h_prev"].view(R, H), slabs, n_split, off[f"nn.weight_hh_l{k}"], off[f"nn.bias_hh_l{k}"])
            d_h = ops.dense_dgrad(dg, views[f"nn.weight_ih_l{k}"]).view(B, L, H)
        ops.dense_wgrad(d_h.view(R, H), obs.view(R, self.obs_dim), slabs, n_split, off["fc1.weight"], off["fc1.bias"])
        return slabs


# ---- the continuous-action nets (utils/net/continuous.py) ---------------------------------------------------------------
class _ContinuousNet(FlatMLP):
    """A `FlatMLP` under the reference's `Net(hidden_sizes=[...])` + `last` key names."""

    ref_scheme = "head"


class ContinuousActorDeterministic(_ContinuousNet):
    """continuous.py:32-88: obs -> hidden ... -> act_dim raw outputs; the action is `max_action * tanh(raw)`
    (`ops.cac_det_action`), which `forward` does NOT apply: the learners need the raw output for the backward."""

    def __init__(self, obs_dim: int, act_dim: int, hidden_sizes=(64, 64), max_action: float = 1.0, act: str = "relu",
                 device: str | torch.device = "cuda", seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        ops.cac_check(int(act_dim))
        super().__init__([int(obs_dim), *[int(h) for h in hidden_sizes], int(act_dim)], act, device=device, seed=seed,
                         storage=storage)
        self.max_action = float(max_action)
        self.act_dim = int(act_dim)


class ContinuousCritic(_ContinuousNet):
    """continuous.py:102-175: rows [obs | act] -> hidden ... -> 1."""

    def __init__(self, obs_dim: int, act_dim: int, hidden_sizes=(64, 64), act: str = "relu",
                 device: str | torch.device = "cuda", seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        super().__init__([int(obs_dim) + int(act_dim), *[int(h) for h in hidden_sizes], 1], act, device=device, seed=seed,
                         storage=storage)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)


class ContinuousActorProbabilistic(_ContinuousNet):
    """continuous.py:178-247.  `conditioned_sigma=True`: the reference's `mu` and `sigma` heads (one Linear each on the shared
    trunk) are ONE last layer of 2 act_dim outputs, [mu_raw | sigma_raw]; a checkpoint carries its two halves as `mu.model.0.*`
    and `sigma.model.0.*`.  `conditioned_sigma=False` (the reference's default): the net emits mu_raw alone and the
    state-independent `sigma_param` (zeros at first, continuous.py:222) is the last act_dim entries of the flat parameter, behind
    the layers, so that one Adam steps both.  The tanh on mu, the clamp and exp on sigma are `ops.sac_action`'s."""

    def __init__(self, obs_dim: int, act_dim: int, hidden_sizes=(64, 64), max_action: float = 1.0, unbounded: bool = False,
                 conditioned_sigma: bool = False, act: str = "relu", device: str | torch.device = "cuda",
                 seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        ops.cac_check(int(act_dim))
        Ad, cond = int(act_dim), bool(conditioned_sigma)
        dims = [int(obs_dim), *[int(h) for h in hidden_sizes], 2 * Ad if cond else Ad]
        # the layers view the head of the vector, sigma_param its tail
        super().__init__(dims, act, device=device, seed=seed, storage=storage, n_extra=0 if cond else Ad)
        self.flat.data[self.n_mlp_params:].zero_()
        if unbounded and not np.isclose(max_action, 1.0):
            max_action = 1.0   # continuous.py:208-210: discarded when unbounded
        self.max_action, self.unbounded, self.act_dim, self.conditioned_sigma = float(max_action), bool(unbounded), Ad, cond

    @property
    def sigma_param(self) -> torch.Tensor | None:
        """f32 [act_dim]: a view of the flat parameter's tail (None with conditioned sigma)."""
        return None if self.conditioned_sigma else self.flat.data[self.n_mlp_params:]

    def param_views(self, flat: torch.Tensor | None = None) -> list[torch.Tensor]:
        """The layers, whole, then `sigma_param` where the vector has it: the vector's order, which is not the checkpoint's."""
        flat = self._vector(flat)
        tail = [] if self.conditioned_sigma else [flat[self.n_mlp_params:].view(self.act_dim, 1)]
        return [v for Wb in self.layer_views(flat) for v in Wb] + tail

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """The reference's state_dict order: a module's own parameters come before its submodules', so `sigma_param` leads;
        then the trunk, then the last layer as `mu` (with conditioned sigma: its halves as `mu` and `sigma`)."""
        Ad = self.act_dim
        trunk = super().reference_named_views(flat)[:-2]
        W, b = self.layer_views(self._vector(flat))[-1]
        if self.conditioned_sigma:
            return trunk + [("mu.model.0.weight", W[:Ad]), ("mu.model.0.bias", b[:Ad]), ("sigma.model.0.weight", W[Ad:]),
                            ("sigma.model.0.bias", b[Ad:])]
        return [("sigma_param", self.param_views(flat)[-1])] + trunk + [("mu.model.0.weight", W), ("mu.model.0.bias", b)]


class Perturbation(_ContinuousNet):
    """continuous.py:395-432: BCQ's perturbation net, rows [obs | act] -> hidden ... -> act_dim raw outputs, with the two
    constants of its epilogue `clamp(act + phi * max_action * tanh(raw), +-max_action)` (`ops.bcq_perturb`, which `forward`
    does NOT apply: the learner needs the raw output for the backward).  The reference's `preprocess_net` is a
    `Net(hidden_sizes=[...])`; a checkpoint carries the layers under `preprocess_net.model.model.{2 i}`."""

    ref_scheme = "body"

    def __init__(self, *, obs_dim: int, act_dim: int, hidden_sizes=(64, 64), max_action: float = 1.0, phi: float = 0.05,
                 act: str = "relu", device: str | torch.device = "cuda", seed: int | None = None,
                 storage: torch.Tensor | None = None) -> None:
        ops.bcq_check(int(act_dim))
        super().__init__([int(obs_dim) + int(act_dim), *[int(h) for h in hidden_sizes], int(act_dim)], act, device=device,
                         seed=seed, storage=storage)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.max_action, self.phi = float(max_action), float(phi)

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        return [("preprocess_net." + k, v) for k, v in super().reference_named_views(flat)]


class VAE(FlatNet):
    """continuous.py:435-513: BCQ's conditional VAE of the action on ONE flat f32 vector [encoder | decoder].  The reference's
    encoder (an `MLP` that ends in its activation) and its two linear heads `mean` and `log_std` are ONE `FlatMLP`
    [D + Ad, *encoder_hidden_sizes, 2 L]: rows [0, L) of its last layer are `mean`, rows [L, 2 L) `log_std`, so one forward, one
    backward and one `input_grad` serve the three modules and the head's output is [mean | raw log_std].  The decoder is a
    `FlatMLP` [D + L, *decoder_hidden_sizes, Ad].  So the vector's order is not the reference's `parameters()` order (there
    mean.weight, mean.bias, log_std.weight, log_std.bias follow one another); `reference_named_views` gives its keys as views.
    The latent, the loss and their gradients are csrc/bcq.hip's; `forward` takes the normals as an argument."""

    def __init__(self, *, encoder_hidden_sizes=(750, 750), decoder_hidden_sizes=(750, 750), obs_dim: int, act_dim: int,
                 latent_dim: int, max_action: float = 1.0, act: str = "relu", device: str | torch.device = "cuda",
                 seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        super().__init__()
        D, Ad, L = self.obs_dim, self.act_dim, self.latent_dim = int(obs_dim), int(act_dim), int(latent_dim)
        ops.bcq_check(Ad, L)
        if not len(encoder_hidden_sizes):
            raise ValueError("VAE: the encoder needs a hidden layer (the reference's hidden_dim feeds the mean and log_std heads)")
        self.max_action, self.act = float(max_action), act
        enc_dims = [D + Ad, *[int(h) for h in encoder_hidden_sizes], 2 * L]
        dec_dims = [D + L, *[int(h) for h in decoder_hidden_sizes], Ad]
        self.n_enc = ops.mlp_param_count(ops.mlp_desc(enc_dims, act))
        n_dec = ops.mlp_param_count(ops.mlp_desc(dec_dims, act))
        storage = self._claim(self.n_enc + n_dec, storage, device)
        self.encoder = FlatMLP(enc_dims, act, device=storage.device, seed=seed, storage=storage[:self.n_enc])
        self.decoder = FlatMLP(dec_dims, act, device=storage.device, seed=None if seed is None else seed + 1,
                               storage=storage[self.n_enc:])
        self.dims = [D + Ad, Ad]

    def rebind(self, storage: torch.Tensor) -> None:
        storage.copy_(self.flat.data)
        self.flat = nn.Parameter(storage, requires_grad=False)
        self.encoder.rebind(storage[:self.n_enc])
        self.decoder.rebind(storage[self.n_enc:])

    def param_views(self, flat: torch.Tensor | None = None) -> list[torch.Tensor]:
        """The layers in the vector's order: the encoder's, its last one whole ([mean | log_std]), then the decoder's."""
        flat = self._vector(flat)
        return [v for net, part in ((self.encoder, flat[:self.n_enc]), (self.decoder, flat[self.n_enc:]))
                for Wb in net.layer_views(part) for v in Wb]

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """`encoder.model.{2 i}`, `mean`, `log_std`, `decoder.model.{2 i}`: the reference module's `state_dict()` order."""
        flat, L, enc = self._vector(flat), self.latent_dim, self.encoder
        trunk = enc.named_layers(ref_layer_keys(enc.n_layers - 1, "seq"), "encoder.model.", flat[:self.n_enc])
        W, b = enc.layer_views(flat[:self.n_enc])[-1]
        heads = [("mean.weight", W[:L]), ("mean.bias", b[:L]), ("log_std.weight", W[L:]), ("log_std.bias", b[L:])]
        return trunk + heads + self.decoder.named_layers(ref_layer_keys(self.decoder.n_layers, "seq"), "decoder.model.",
                                                         flat[self.n_enc:])

    def forward(self, obs: torch.Tensor, act: torch.Tensor, eps: torch.Tensor, save: bool = True):
        """obs [B, D], act [B, Ad], eps [B, L] standard normals (`torch.randn_like(std)`, continuous.py:493)
        -> (recon [B, Ad], mean [B, L], std [B, L]); with `save` the decoder's raw output, the head's and eps stay for
        `backward`."""
        dev = self.flat.device
        obs = obs.to(dev, torch.float32).reshape(-1, self.obs_dim).contiguous()
        act = act.to(dev, torch.float32).reshape(obs.shape[0], self.act_dim).contiguous()
        eps = eps.to(dev, torch.float32).reshape(obs.shape[0], self.latent_dim).contiguous()
        head, raw, std = self.forward_rows(ops.maddpg_joint_rows([obs], [act]), obs, eps, save=save)
        return ops.cac_det_action(raw, self.max_action), head[:, :self.latent_dim], std

    def forward_rows(self, x: torch.Tensor, obs: torch.Tensor, eps: torch.Tensor, save: bool = True):
        """`forward` for a caller that has the rows x = [obs | act] already and needs no `recon` (the learner: `loss_head`
        forms it again from the raw output) -> (head [B, 2 L], the decoder's raw output [B, Ad], std [B, L])."""
        head = FlatMLP.forward(self.encoder, x, save=save)
        x_dec, std = ops.bcq_latent(head, eps, obs)
        raw = FlatMLP.forward(self.decoder, x_dec, save=save)
        if save:
            self._saved = (head, eps, raw)
        return head, raw, std

    def decode_rows(self, x: torch.Tensor) -> torch.Tensor:
        """The decoder on rows [obs | z] that are already assembled (`ops.bcq_decode_rows`, `ops.bcq_latent`) -> its raw
        output [n, Ad]; the action is `max_action * tanh(raw)` (`ops.bcq_action_rows`).  Nothing is kept."""
        return FlatMLP.forward(self.decoder, x, save=False)

    def loss_head(self, act: torch.Tensor) -> dict:
        """`ops.bcq_vae_head` on the last `forward(save=True)`: dict(d_raw, partial)."""
        head, _, raw = self._saved_forward("loss_head")
        return ops.bcq_vae_head(raw, act, head, self.max_action)

    def backward(self, d_raw: torch.Tensor, n_split: int = 0, slabs: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient slabs [n_split, n_param] of vae_loss for the last `forward(save=True)`, d_raw = `loss_head`'s: the
        decoder's slabs and its gradient to the latent columns, `ops.bcq_latent_grad` (the KL term enters there), the
        encoder's slabs."""
        head, eps, raw = self._saved_forward()
        P = self.flat.numel()
        n_split, slabs = self._slabs(raw.shape[0], n_split, slabs)
        d_raw = d_raw.reshape(raw.shape).contiguous()
        self.decoder.backward(d_raw, n_split, slabs=slabs[:, self.n_enc:], slab_stride=P)
        dz = self.decoder.input_grad(d_raw, self.obs_dim, self.latent_dim)
        self.encoder.backward(ops.bcq_latent_grad(dz, head, eps), n_split, slabs=slabs, slab_stride=P)
        return slabs


class _GroupedLayers:
    """`EnsembleLinear`'s layout (common.py:522-554) of `E` members of the chain `dims` on `net`'s flat vector from `offset`
    on: per layer weight [E, in, out], then bias [E, 1, out] -- what csrc/ensemble.hip runs as one grouped launch per layer."""

    def __init__(self, net: FlatNet, dims, E: int, offset: int = 0) -> None:
        self.net, self.dims, self.E = net, list(dims), int(E)
        self.offsets, o = [], offset
        for k, m in zip(self.dims, self.dims[1:]):
            self.offsets.append((o, o + E * k * m))
            o += E * (k * m + m)
        self.n_param = o - offset

    @property
    def n_layers(self) -> int:
        return len(self.dims) - 1

    def weight(self, i: int, flat: torch.Tensor | None = None) -> torch.Tensor:
        """Layer i's weight [E, in, out], a view of the net's vector (or of any vector of its layout, e.g. a gradient)."""
        o, ob = self.offsets[i]
        return self.net._vector(flat)[o:ob].view(self.E, self.dims[i], self.dims[i + 1])

    def bias(self, i: int, flat: torch.Tensor | None = None) -> torch.Tensor:
        """Layer i's bias [E, 1, out]."""
        _, ob = self.offsets[i]
        return self.net._vector(flat)[ob:ob + self.E * self.dims[i + 1]].view(self.E, 1, self.dims[i + 1])

    @torch.no_grad()
    def reset(self, seed: int | None, bound) -> None:
        """Uniform +-bound(in) for the weight and for the bias, layer by layer.  The draw is EnsembleLinear's `rand * 2 k - k`
        (common.py:541-548), whose bits are not `_uniform`'s; `bound` is the caller's, to the last bit of its own spelling."""
        gen = _generator(seed)
        for i in range(self.n_layers):
            k = bound(self.dims[i])
            for v in (self.weight(i), self.bias(i)):
                v.copy_(torch.rand(v.shape, generator=gen) * 2 * k - k)


class EnsembleCritic(FlatNet):
    """An ensemble of `ensemble_size` critics [obs | act] -> hidden ... -> 1 of one shape, the reference's
    `ContinuousCritic(preprocess_net=Net(..., linear_layer=EnsembleLinear), linear_layer=EnsembleLinear, flatten_input=False)`
    (utils/net/common.py:522-554, continuous.py:102-175; examples/mujoco/mujoco_redq.py), as ONE flat HBM vector in the
    reference's `parameters()` order -- per layer weight [E, in, out], then bias_weights [E, 1, out] -- so a reference
    checkpoint is a set of views of it.  forward / backward / input_grad run in csrc/ensemble.hip: one grouped launch per
    layer and role serves all members.  `forward` -> [E, B, 1]."""

    def __init__(self, obs_dim: int, act_dim: int, ensemble_size: int, hidden_sizes=(64, 64), act: str = "relu",
                 device: str | torch.device = "cuda", seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        super().__init__()
        self.obs_dim, self.act_dim, self.ensemble_size = int(obs_dim), int(act_dim), int(ensemble_size)
        self.dims = [self.obs_dim + self.act_dim, *[int(h) for h in hidden_sizes], 1]
        self.act = act
        self.desc = ops.mlp_desc(self.dims, act)
        self._layers = _GroupedLayers(self, self.dims, self.ensemble_size)
        assert self._layers.n_param == ops.ens_mlp_param_count(self.desc, self.ensemble_size)
        self._claim(self._layers.n_param, storage, device)
        self.reset_parameters(seed)

    @property
    def n_layers(self) -> int:
        return len(self.dims) - 1

    def weight(self, i: int, flat: torch.Tensor | None = None) -> torch.Tensor:
        """Layer i's weight [E, in, out], a view of the flat vector (or of any vector of its layout, e.g. a gradient)."""
        return self._layers.weight(i, flat)

    def bias(self, i: int, flat: torch.Tensor | None = None) -> torch.Tensor:
        """Layer i's bias_weights [E, 1, out]."""
        return self._layers.bias(i, flat)

    def reset_parameters(self, seed: int | None = None) -> None:
        """EnsembleLinear's init (common.py:541-548): uniform +-sqrt(1 / in) for the weight and for the bias."""
        self._layers.reset(seed, lambda k: math.sqrt(1.0 / k))

    def forward(self, x: torch.Tensor, save: bool = True) -> torch.Tensor:
        """x [B, obs_dim + act_dim], shared by all members -> Q [E, B, 1]."""
        x = x.to(self.flat.device, torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != self.dims[0]:
            raise ValueError(f"EnsembleCritic: input must be [B, {self.dims[0]}], got {list(x.shape)}")
        out, acts = ops.ens_mlp_forward(self.desc, self.ensemble_size, self.flat.data, x)
        if save:
            self._saved = (x, acts)
        return out

    def backward(self, d_out: torch.Tensor, n_split: int = 0, slabs: torch.Tensor | None = None,
                 slab_stride: int = 0) -> torch.Tensor:
        """Gradient slabs [n_split, n_param] of sum(out * d_out), d_out [E, B(, 1)], for the last `forward(save=True)`."""
        x, acts = self._saved_forward()
        return ops.ens_mlp_backward(self.desc, self.ensemble_size, self.flat.data, x, acts, d_out.contiguous(), n_split,
                                    slabs=slabs, slab_stride=slab_stride)

    def input_grad(self, d_out: torch.Tensor, col0: int, n_col: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient [B, n_col] of sum(out * d_out) w.r.t. the input columns [col0, col0 + n_col) of the last
        `forward(save=True)`, summed over the members in order; no weight gradient is computed."""
        x, acts = self._saved_forward("input_grad")
        return ops.ens_mlp_input_grad(self.desc, self.ensemble_size, self.flat.data, x, acts, d_out.contiguous(), col0, n_col,
                                      out=out)

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """`Net` + `last` key names, an EnsembleLinear's bias being its `bias_weights`."""
        return [kv for i, (kw, kb) in enumerate(ref_layer_keys(self.n_layers, "head"))
                for kv in ((kw, self.weight(i, flat)), (kb + "_weights", self.bias(i, flat)))]


class ImplicitQuantileNet(FlatNet):
    """ImplicitQuantileNetwork (discrete.py:164-217) on ONE flat f32 parameter vector in the reference module's
    `parameters()` order: the preprocess layers, the `last` layers, then the cosine embedding's weight [H, C] and bias [H].
    `preprocess` (obs -> ... -> H) and `last` (H -> hidden_sizes -> A) are `FlatMLP`s over slices of the vector (csrc/dense.hip);
    the embedding and its product with the features are csrc/iqn.hip.  `feature_act`: the preprocess net ends in its
    activation, as the reference's `Net` does (every hidden layer is followed by one); the ReLU is then applied inside the
    embedding kernels.  A network row is (b, s): `forward` returns out [R * S, A], the reference's [R, A, S] logits being
    `out.view(R, S, A).transpose(1, 2)`."""

    split_optimizer_state = False

    def __init__(self, preprocess_dims, n_act: int, hidden_sizes=(), num_cosines: int = 64, act: str = "relu",
                 feature_act: bool = True, device: str | torch.device = "cuda", seed: int | None = None,
                 storage: torch.Tensor | None = None) -> None:
        super().__init__()
        if act != "relu":
            raise ValueError("ImplicitQuantileNet: the embedding kernels carry the ReLU of the reference; act must be 'relu'")
        self.pre_dims = [int(d) for d in preprocess_dims]
        self.n_act, self.hidden_sizes, self.num_cosines = int(n_act), tuple(int(h) for h in hidden_sizes), int(num_cosines)
        self.act, self.feature_act = act, bool(feature_act)
        H = self.embedding_dim = self.pre_dims[-1]
        ops.iqn_check(self.num_cosines, H, 2, self.n_act)
        self.last_dims = [H, *self.hidden_sizes, self.n_act]
        n_pre = ops.mlp_param_count(ops.mlp_desc(self.pre_dims, act))
        n_last = ops.mlp_param_count(ops.mlp_desc(self.last_dims, act))
        self.w_off, self.b_off = n_pre + n_last, n_pre + n_last + H * self.num_cosines
        storage = self._claim(self.b_off + H, storage, device)
        self.n_pre, self.n_last = n_pre, n_last
        self.preprocess = FlatMLP(self.pre_dims, act, device=storage.device, seed=seed, storage=storage[:n_pre])
        self.last = FlatMLP(self.last_dims, act, device=storage.device, seed=None if seed is None else seed + 1,
                            storage=storage[n_pre:n_pre + n_last])
        self.dims = [self.pre_dims[0], self.n_act]   # what the policies ask of a Q-network: input width, outputs per sample
        self.reset_embedding(None if seed is None else seed + 2)

    def _embedding(self, flat: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        flat = self._vector(flat)
        return flat[self.w_off:self.b_off].view(self.embedding_dim, self.num_cosines), flat[self.b_off:]

    @property
    def We(self) -> torch.Tensor:
        return self._embedding()[0]

    @property
    def be(self) -> torch.Tensor:
        return self._embedding()[1]

    @torch.no_grad()
    def reset_embedding(self, seed: int | None = None) -> None:
        """torch nn.Linear default init of the embedding layer."""
        gen = _generator(seed)
        bound = 1.0 / math.sqrt(self.num_cosines)
        self.We.copy_(_uniform(self.We.shape, bound, gen))
        self.be.copy_(_uniform(self.be.shape, bound, gen))

    def forward(self, x: torch.Tensor, sample_size: int, taus: torch.Tensor | None = None, save: bool = True, seed: int = 0,
                offset: int = 0, offset_dev: torch.Tensor | None = None):
        """x [R, D] -> (out [R * S, A], taus [R, S]).  taus None: drawn on the device (tsm_iqn_taus at `seed`, `offset`,
        `offset_dev`); given: used as they are."""
        x = x.to(self.flat.device, torch.float32).contiguous().reshape(-1, self.pre_dims[0])
        R, S = x.shape[0], int(sample_size)
        ops.iqn_check(self.num_cosines, self.embedding_dim, S, self.n_act)
        if taus is None:
            taus = ops.iqn_taus(R, S, seed, x.device, offset=offset, offset_dev=offset_dev)
        elif tuple(taus.shape) != (R, S):
            raise ValueError(f"ImplicitQuantileNet: taus must be [{R}, {S}]")
        taus = taus.to(self.flat.device, torch.float32).contiguous()
        f = FlatMLP.forward(self.preprocess, x, save=save)
        e, phi = ops.iqn_embed_forward(f, taus, self.We, self.be, relu_f=self.feature_act)
        out = FlatMLP.forward(self.last, e, save=save)
        if save:
            self._saved = (f, phi, taus)
        return out, taus

    def backward(self, d_out: torch.Tensor, n_split: int = 0, slabs: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient slabs [n_split, n_param] of the whole flat vector for the last `forward(save=True)`, in one pass:
        `last`'s weight slabs, its input gradient (a second walk of its dgrad chain: `FlatMLP.input_grad`), the embedding's
        backward, the preprocess net's slabs."""
        f, phi, taus = self._saved_forward()
        R, S = taus.shape
        P = self.flat.numel()
        n_split, slabs = self._slabs(R, n_split, slabs)
        d_out = d_out.reshape(R * S, self.n_act).contiguous()
        self.last.backward(d_out, n_split, slabs=slabs[:, self.n_pre:], slab_stride=P)
        d_e = self.last.input_grad(d_out, 0, self.embedding_dim)
        d_f, _ = ops.iqn_embed_backward(d_e, f, phi, taus, self.We, self.be, n_split, slabs=slabs, slab_stride=P,
                                        w_off=self.w_off, b_off=self.b_off, relu_f=self.feature_act)
        self.preprocess.backward(d_f, n_split, slabs=slabs, slab_stride=P)
        return slabs

    # ---- reference checkpoint compatibility ---------------------------------------------------------------------------
    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """`preprocess.model.model.{2 i}` (Net: Linear, activation, ...), `last.model.{2 i}` (MLP), `embed_model.net.0`
        (tests/golden/iqn.npz, sd_*)."""
        flat = self._vector(flat)
        We, be = self._embedding(flat)
        return (self.preprocess.named_layers(ref_layer_keys(self.preprocess.n_layers, "body"), "preprocess.", flat[:self.n_pre])
                + self.last.named_layers(ref_layer_keys(self.last.n_layers, "seq"), "last.model.", flat[self.n_pre:self.w_off])
                + [("embed_model.net.0.weight", We), ("embed_model.net.0.bias", be)])


class FractionProposalNet(FlatNet):
    """FractionProposalNetwork (discrete.py:220-253) on ONE flat f32 vector [N * H + N]: the linear layer's weight [N, H], then
    its bias [N]; softmax, cumulative sum and entropy are csrc/fqf.hip.  `feature_act` as `ImplicitQuantileNet`'s: `forward`
    takes the preprocess net's last LINEAR output and the kernels apply its ReLU."""

    split_optimizer_state = False

    def __init__(self, num_fractions: int, embedding_dim: int, feature_act: bool = True, device: str | torch.device = "cuda",
                 seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        super().__init__()
        N, H = self.num_fractions, self.embedding_dim = int(num_fractions), int(embedding_dim)
        ops.fqf_check(N, H)
        self.feature_act = bool(feature_act)
        self._claim(N * H + N, storage, device)
        self.reset_parameters(seed)

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        flat, N, H = self._vector(flat), self.num_fractions, self.embedding_dim
        return [("net.weight", flat[:N * H].view(N, H)), ("net.bias", flat[N * H:])]

    @property
    def Wf(self) -> torch.Tensor:
        return self.reference_named_views()[0][1]

    @property
    def bf(self) -> torch.Tensor:
        return self.reference_named_views()[1][1]

    @torch.no_grad()
    def reset_parameters(self, seed: int | None = None) -> None:
        """discrete.py:235-236: xavier_uniform_(gain=0.01) weight, zero bias."""
        bound = 0.01 * math.sqrt(6.0 / (self.embedding_dim + self.num_fractions))
        self.Wf.copy_(_uniform(self.Wf.shape, bound, _generator(seed)))
        self.bf.zero_()

    def forward(self, f: torch.Tensor, save: bool = True):
        """f [R, H] -> (taus [R, N + 1], tau_hats [R, N], logp [R, N], entropies [R])."""
        f = f.to(self.flat.device, torch.float32).contiguous().reshape(-1, self.embedding_dim)
        if save:
            self._saved = f
        return ops.fqf_propose(f, self.Wf, self.bf, relu_f=self.feature_act)

    def backward(self, d_logits: torch.Tensor, n_split: int = 0, slabs: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient slabs [n_split, N * H + N] for the features of the last `forward(save=True)`."""
        return ops.fqf_propose_backward(d_logits, self._saved_forward(), n_split, slabs=slabs, relu_f=self.feature_act)


class FullQuantileNet(ImplicitQuantileNet):
    """FullQuantileFunction (discrete.py:256-315): an `ImplicitQuantileNet` evaluated where a `FractionProposalNet` says."""

    def forward(self, x: torch.Tensor, propose_model: FractionProposalNet, fractions: Batch | None = None,  # type: ignore[override]
                save: bool = True, training: bool = False):
        """x [R, D] -> (out [R * N, A] at tau_hats, fractions = Batch(taus, tau_hats, entropies, logp), out_tau
        [R * (N - 1), A] at taus[:, 1:-1] when `training`, else None).  The preprocess net runs once; `fractions` None: proposed
        on its features.  With `save` the forward at tau_hats is the one `backward` differentiates; the interior pass keeps
        nothing."""
        x = x.to(self.flat.device, torch.float32).contiguous().reshape(-1, self.pre_dims[0])
        f = FlatMLP.forward(self.preprocess, x, save=save)
        if fractions is None:
            taus, tau_hats, logp, entropies = propose_model.forward(f, save=save)
            fractions = Batch(taus=taus, tau_hats=tau_hats, entropies=entropies, logp=logp)
        taus, tau_hats = fractions.taus, fractions.tau_hats
        R, N = x.shape[0], tau_hats.shape[1]
        if tuple(tau_hats.shape) != (R, N) or tuple(taus.shape) != (R, N + 1):
            raise ValueError(f"FullQuantileNet: fractions must hold taus [{R}, N + 1] and tau_hats [{R}, N]")
        ops.fqf_check(N, self.embedding_dim, self.n_act)
        e, phi = ops.iqn_embed_forward(f, tau_hats, self.We, self.be, relu_f=self.feature_act)
        out = FlatMLP.forward(self.last, e, save=save)
        if save:
            self._saved = (f, phi, tau_hats.contiguous())
        out_tau = None
        if training:
            e_tau, _ = ops.iqn_embed_forward(f, taus[:, 1:-1].contiguous(), self.We, self.be, relu_f=self.feature_act)
            out_tau = FlatMLP.forward(self.last, e_tau, save=False)
        return out, fractions, out_tau


# ---- the learned global states of CTDE (algorithm/multiagent/ctde.py:268-280, 302-335) ------------------------------------------
class _StateNet(FlatNet):
    """What the two learned `GlobalStateConstructor` modes share: joint rows obs [R, N, D] -> state [R, hidden_dim], two
    `FlatMLP`s `head` and `tail` over consecutive slices of the vector around a kernel of csrc/gstate.hip that folds the agents."""

    def _build(self, head_dims, head_act: str, tail_dims, storage, device, seeds) -> None:
        n_head = ops.mlp_param_count(ops.mlp_desc(head_dims, head_act))
        n_tail = ops.mlp_param_count(ops.mlp_desc(tail_dims, "none"))
        storage = self._claim(n_head + n_tail, storage, device)
        self.n_head = n_head
        self.head = FlatMLP(head_dims, head_act, device=storage.device, seed=seeds[0], storage=storage[:n_head])
        self.tail = FlatMLP(tail_dims, "none", device=storage.device, seed=seeds[1], storage=storage[n_head:])
        self.dims = [self.n_agents * self.obs_dim, self.hidden_dim]   # a critic's input is dims[-1] wide

    def rebind(self, storage: torch.Tensor) -> None:
        self.flat = nn.Parameter(storage, requires_grad=False)
        self.head.rebind(storage[:self.n_head])
        self.tail.rebind(storage[self.n_head:])

    def _rows(self, obs: torch.Tensor) -> tuple[torch.Tensor, int]:
        N, D = self.n_agents, self.obs_dim
        obs = obs.to(self.flat.device, torch.float32).contiguous()
        if obs.dim() < 2 or obs.numel() == 0 or obs.numel() % (N * D) or (obs.dim() == 3 and tuple(obs.shape[1:]) != (N, D)):
            raise ValueError(f"{type(self).__name__}: obs must be [R, {N}, {D}] (or [R, {N * D}], agents in order), got "
                             f"{list(obs.shape)}")
        return obs.reshape(-1, D), obs.numel() // (N * D)

    def _fold(self, y: torch.Tensor, R: int):
        """The head's output y [R N, .] -> (the tail's input [R, .], what `_unfold` needs)."""
        raise NotImplementedError

    def _unfold(self, d_x: torch.Tensor, y: torch.Tensor, kept) -> torch.Tensor:
        """The gradient of the tail's input -> the gradient of the head's output [R N, .]."""
        raise NotImplementedError

    def forward(self, obs: torch.Tensor, save: bool = True) -> torch.Tensor:
        """obs [R, N, D], agents in env.agents order -> [R, hidden_dim]."""
        x, R = self._rows(obs)
        y = FlatMLP.forward(self.head, x, save=save)
        z, kept = self._fold(y, R)
        out = FlatMLP.forward(self.tail, z, save=save)
        if save:
            self._saved = (y, kept, R)
        return out

    def backward(self, d_state: torch.Tensor, n_split: int = 0, slabs: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient slabs [n_split, n_param] of sum(state * d_state) for the last `forward(save=True)`: the tail's slabs and
        its input gradient, the fold's backward, the head's slabs."""
        y, kept, R = self._saved_forward()
        P = self.flat.numel()
        n_split, slabs = self._slabs(R, n_split, slabs)
        d_state = d_state.to(self.flat.device, torch.float32).reshape(R, self.hidden_dim).contiguous()
        self.tail.backward(d_state, n_split, slabs=slabs[:, self.n_head:], slab_stride=P)
        d_x = self.tail.input_grad(d_state, 0, self.tail.dims[0])
        self.head.backward(self._unfold(d_x, y, kept), n_split, slabs=slabs, slab_stride=P)
        return slabs


class AttentionStateNet(_StateNet):
    """`GlobalStateConstructor(mode="attention")` (ctde.py:268-275, 302-312): nn.MultiheadAttention(embed_dim=obs_dim,
    num_heads=4, batch_first=True) over the agents, the mean over agents, Linear(obs_dim, hidden_dim) -- on ONE flat f32 vector
    in the module's `parameters()` order.  The in-projection is the `FlatMLP` [D, 3 D] `head`; the out-projection and
    `output_proj` are the two linear layers of the `FlatMLP` [D, D, hidden_dim] `tail`, which runs on the POOLED rows (the mean
    commutes with a linear layer); between them tsm_attn_pool_forward / _backward.  No mask, no dropout."""

    def __init__(self, obs_dim: int, n_agents: int, hidden_dim: int = 64, device: str | torch.device = "cuda",
                 seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        super().__init__()
        self.obs_dim, self.n_agents, self.hidden_dim = int(obs_dim), int(n_agents), int(hidden_dim)
        ops.gstate_check(self.n_agents, self.obs_dim)
        D = self.obs_dim
        self._build([D, 3 * D], "none", [D, D, self.hidden_dim], storage, device, (0, 0))
        self.reset_parameters(seed)

    @torch.no_grad()
    def reset_parameters(self, seed: int | None = None) -> None:
        """torch's own: xavier-uniform in_proj_weight, zero in_proj_bias and out_proj.bias (nn.MultiheadAttention
        ._reset_parameters), nn.Linear's default for out_proj.weight and for output_proj."""
        gen, D = _generator(seed), self.obs_dim
        views = dict(self.reference_named_views())
        views["attention.in_proj_weight"].copy_(_uniform((3 * D, D), math.sqrt(6.0 / (4 * D)), gen))
        views["attention.in_proj_bias"].zero_()
        views["attention.out_proj.weight"].copy_(_uniform((D, D), 1.0 / math.sqrt(D), gen))
        views["attention.out_proj.bias"].zero_()
        for k in ("output_proj.weight", "output_proj.bias"):
            views[k].copy_(_uniform(views[k].shape, 1.0 / math.sqrt(D), gen))

    def _fold(self, qkv: torch.Tensor, R: int):
        return ops.attn_pool_forward(qkv.view(R, self.n_agents, 3 * self.obs_dim), self.n_agents)

    def _unfold(self, d_ctx: torch.Tensor, qkv: torch.Tensor, P: torch.Tensor) -> torch.Tensor:
        return ops.attn_pool_backward(d_ctx, qkv.view(P.shape[0], self.n_agents, 3 * self.obs_dim), P).view(qkv.shape)

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        flat = self._vector(flat)
        return (self.head.named_layers([("attention.in_proj_weight", "attention.in_proj_bias")], flat=flat[:self.n_head])
                + self.tail.named_layers([("attention.out_proj.weight", "attention.out_proj.bias"),
                                          ("output_proj.weight", "output_proj.bias")], flat=flat[self.n_head:]))


def agent_pool_coefficients(n_agents: int, adjacency_matrix=None) -> np.ndarray:
    """float64 [N]: c_m = (1 / N) sum_n A^[n][m] with A^ the row-normalised adjacency (ctde.py:323-326); None: the plain mean
    (:329), c_m = 1 / N.  ValueError unless the adjacency is [N, N], finite, non-negative, with every row sum > 0 (the reference
    divides by the row sum and would return inf / nan)."""
    N = int(n_agents)
    if adjacency_matrix is None:
        return np.full(N, 1.0 / N, np.float64)
    A = adjacency_matrix.detach().cpu().numpy() if isinstance(adjacency_matrix, torch.Tensor) else np.asarray(adjacency_matrix)
    A = A.astype(np.float64)
    if A.shape != (N, N):
        raise ValueError(f"adjacency_matrix must be [{N}, {N}], got {list(A.shape)}")
    if not np.isfinite(A).all() or (A < 0).any():
        raise ValueError("adjacency_matrix must be finite and non-negative")
    rows = A.sum(axis=1)
    if not (rows > 0).all():
        raise ValueError(f"adjacency_matrix: every row sum must be > 0; rows {np.nonzero(~(rows > 0))[0].tolist()} have none")
    return (A / rows[:, None]).sum(axis=0) / N


class GraphStateNet(_StateNet):
    """`GlobalStateConstructor(mode="graph")` (ctde.py:277-280, 314-335): relu(gnn_layer1(obs)) per agent, neighbour aggregation
    by the row-normalised adjacency (or the plain mean), gnn_layer2, the mean over agents -- on ONE flat f32 vector in the
    module's `parameters()` order.  gnn_layer1 is the `FlatMLP` [D, H] `head` (its ReLU is applied by the pool kernels: a
    `FlatMLP` ends linear), gnn_layer2 the `FlatMLP` [H, H] `tail` on the pooled rows: aggregation and mean are ONE weighted sum
    over the agents with the coefficients `c` (`agent_pool_coefficients`), which commutes with the linear layer."""

    def __init__(self, obs_dim: int, n_agents: int, hidden_dim: int = 64, adjacency_matrix=None,
                 device: str | torch.device = "cuda", seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        super().__init__()
        self.obs_dim, self.n_agents, self.hidden_dim = int(obs_dim), int(n_agents), int(hidden_dim)
        if self.obs_dim < 1 or self.hidden_dim < 1 or not 1 <= self.n_agents <= ops._abi.GSTATE_MAX_AGENTS:
            raise ValueError(f"GraphStateNet: obs_dim = {self.obs_dim}, hidden_dim = {self.hidden_dim} (both at least 1), n_agents = "
                             f"{self.n_agents}; the HIP kernels serve 1 to {ops._abi.GSTATE_MAX_AGENTS} agents")
        self.c64 = agent_pool_coefficients(self.n_agents, adjacency_matrix)
        H = self.hidden_dim
        self._build([self.obs_dim, H], "relu", [H, H], storage, device, (seed, None if seed is None else seed + 1))
        self.c = torch.as_tensor(self.c64.astype(np.float32)).to(self.flat.device)

    def _fold(self, h: torch.Tensor, R: int):
        return ops.agent_pool_forward(h.view(R, self.n_agents, self.hidden_dim), self.c, relu=True), None

    def _unfold(self, d_pool: torch.Tensor, h: torch.Tensor, kept) -> torch.Tensor:
        h3 = h.view(-1, self.n_agents, self.hidden_dim)
        return ops.agent_pool_backward(d_pool, self.c, self.n_agents, h_relu=h3).view(h.shape)

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        flat = self._vector(flat)
        return (self.head.named_layers([("gnn_layer1.weight", "gnn_layer1.bias")], flat=flat[:self.n_head])
                + self.tail.named_layers([("gnn_layer2.weight", "gnn_layer2.bias")], flat=flat[self.n_head:]))


class RainbowNet(FlatNet):
    """The reference's `Net(num_atoms=N, dueling_param=(Q, V), linear_layer=NoisyLinear)` (common.py:246-369 around
    discrete.py:318-375, as test/discrete/test_rainbow.py:97-107 builds it) on ONE flat f32 vector in the module's
    `parameters()` order: the layers of `model`, then of `Q`, then of `V`; a noisy layer is mu_W, sigma_W, mu_bias, sigma_bias,
    eps_p, eps_q (the noise vectors are `nn.Parameter(requires_grad=False)` there and so belong to the vector), a plain one
    weight, bias.  Before every forward `tsm_noisy_compose` writes the EFFECTIVE weights of all layers into a private vector of
    `FlatMLP` layout; the trunk and the two streams are `FlatMLP`s over slices of it (csrc/dense.hip), joined by the kernels of
    csrc/rainbow.hip.  The softmax over atoms stays in the head kernels: `forward` returns the raw [R, A * N].

    `noisy_std` None: plain linear layers.  `dueling` False: one chain obs -> hidden -> A * N.  Noise acts only in torch
    training mode (`self.training`); in eval mode the net is its `mu`."""

    split_optimizer_state = False

    def __init__(self, obs_dim: int, hidden_sizes, n_act: int, num_atoms: int = 51, q_hidden=(), v_hidden=(),
                 dueling: bool = True, noisy_std: float | None = 0.5, device: str | torch.device = "cuda",
                 seed: int | None = None, storage: torch.Tensor | None = None) -> None:
        super().__init__()
        self.obs_dim, self.n_act, self.num_atoms = int(obs_dim), int(n_act), int(num_atoms)
        self.hidden_sizes = tuple(int(h) for h in hidden_sizes)
        self.q_hidden, self.v_hidden = tuple(int(h) for h in q_hidden), tuple(int(h) for h in v_hidden)
        self.dueling, self.noisy_std = bool(dueling), None if noisy_std is None else float(noisy_std)
        A, N = self.n_act, self.num_atoms
        ops.distq_check(A, N)
        if self.dueling:
            if not self.hidden_sizes:
                raise ValueError("RainbowNet: the dueling streams need a trunk: hidden_sizes must not be empty")
            H = self.hidden_sizes[-1]
            chains = [[self.obs_dim, *self.hidden_sizes], [H, *self.q_hidden, A * N], [H, *self.v_hidden, N]]
        else:
            if self.q_hidden or self.v_hidden:
                raise ValueError("RainbowNet: q_hidden / v_hidden belong to the dueling streams (dueling=False)")
            chains = [[self.obs_dim, *self.hidden_sizes, A * N]]
        self._chains = chains
        noisy = self.noisy_std is not None
        self._layers = [(c[i], c[i + 1], noisy) for c in chains for i in range(len(c) - 1)]
        self.table = ops.noisy_net_table(self._layers)
        ops.rainbow_check(self.table)
        storage = self._claim(int(self.table.P), storage, device)
        # the effective parameters: not trained, not saved -- rewritten by every forward
        self.eff = torch.zeros(int(self.table.P_eff), dtype=torch.float32, device=storage.device)
        self._parts, o = [], 0
        for c in chains:
            n = ops.mlp_param_count(ops.mlp_desc(c, "relu"))
            self._parts.append((o, FlatMLP(c, "relu", device=storage.device, seed=0, storage=self.eff[o:o + n])))
            o += n
        self.trunk = self._parts[0][1]
        self.Q, self.V = (self._parts[1][1], self._parts[2][1]) if self.dueling else (None, None)
        self.dims = [self.obs_dim, A * N]   # what the policies ask of a Q-network: input width, outputs per sample
        self._eff_slabs: dict = {}
        self.reset_parameters(seed)

    # ---- views ------------------------------------------------------------------------------------------------------------
    @property
    def n_slots(self) -> int:
        return int(self.table.n_slots)

    def layer_views(self, flat: torch.Tensor | None = None) -> list[dict]:
        """Per layer {name: view} of `flat` (None: the net's own vector; else any vector of its layout, e.g. a summed
        gradient), in `parameters()` order."""
        flat = self.flat.data if flat is None else flat
        out = []
        for l, (i, o, z) in enumerate(self._layers):
            p = int(self.table.layer[l].off)
            blocks = ([("mu_W", (o, i)), ("sigma_W", (o, i)), ("mu_bias", (o,)), ("sigma_bias", (o,)), ("eps_p", (i,)), ("eps_q", (o,))]
                      if z else [("weight", (o, i)), ("bias", (o,))])
            d = {}
            for name, shp in blocks:
                n = int(np.prod(shp))
                d[name] = flat[p:p + n].view(shp)
                p += n
            out.append(d)
        return out

    def noise(self, flat: torch.Tensor | None = None) -> torch.Tensor:
        """The noise slots in slot order (per noisy layer eps_p then eps_q), as one vector [n_slots]."""
        vs = [v[k].reshape(-1) for v in self.layer_views(flat) for k in ("eps_p", "eps_q") if k in v]
        return torch.cat(vs) if vs else torch.zeros(0, dtype=torch.float32, device=self.flat.device)

    @torch.no_grad()
    def set_noise(self, eps) -> None:
        """Load given noise, slot order as `noise()`: for tests and checkpoints."""
        eps = torch.as_tensor(np.asarray(eps, np.float32) if not isinstance(eps, torch.Tensor) else eps).reshape(-1)
        if eps.numel() != self.n_slots:
            raise ValueError(f"RainbowNet.set_noise: {eps.numel()} values for {self.n_slots} noise slots")
        eps, o = eps.to(self.flat.device, torch.float32), 0
        for v in self.layer_views():
            for k in ("eps_p", "eps_q"):
                if k in v:
                    v[k].copy_(eps[o:o + v[k].numel()])
                    o += v[k].numel()

    def sample(self, seed: int, offset: int = 0, offset_dev: torch.Tensor | None = None) -> None:
        """NoisyLinear.sample of every noisy layer, on the device (tsm_noisy_sample at Philox counter offset + *offset_dev)."""
        if self.n_slots:
            ops.noisy_sample(self.table, self.flat.data, seed, offset=offset, offset_dev=offset_dev)

    @torch.no_grad()
    def reset_parameters(self, seed: int | None = None) -> None:
        """NoisyLinear.reset (discrete.py:351-356: mu uniform in +-1 / sqrt(in), sigma = noisy_std / sqrt(in)) and a first
        draw of the noise as `.f` forms it; plain layers get torch's nn.Linear default."""
        gen = _generator(seed)
        for (i, o, z), v in zip(self._layers, self.layer_views()):
            bound = 1.0 / math.sqrt(i)
            for k in ("mu_W", "mu_bias") if z else ("weight", "bias"):
                v[k].copy_(_uniform(v[k].shape, bound, gen))
            if z:
                v["sigma_W"].fill_(self.noisy_std / math.sqrt(i))
                v["sigma_bias"].fill_(self.noisy_std / math.sqrt(i))
                for k in ("eps_p", "eps_q"):
                    x = torch.randn(v[k].shape, generator=gen)
                    v[k].copy_(x.sign() * x.abs().sqrt())

    # ---- forward / backward -------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, save: bool = True) -> torch.Tensor:
        """x [..., D] -> raw [R, A * N].  The effective weights are composed by `self.training`, then trunk -> features ->
        Q, V -> combine (without dueling: the one chain)."""
        x = x.to(self.flat.device, torch.float32).contiguous().reshape(-1, self.obs_dim)
        training = bool(self.training)
        ops.noisy_compose(self.table, self.flat.data, training, out=self.eff)
        z = FlatMLP.forward(self.trunk, x, save=save)
        if self.dueling:
            f = ops.dueling_features(z)
            q = FlatMLP.forward(self.Q, f, save=save)
            v = FlatMLP.forward(self.V, f, save=save)
            out = ops.dueling_combine(q, v, self.n_act, self.num_atoms)
        else:
            out = z
        if save:
            self._saved = (z, training)
        elif self._saved is not None:
            self._saved = False   # the effective weights are no longer those of the saved forward
        return out

    def backward(self, d_out: torch.Tensor, n_split: int = 0, slabs: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient slabs [n_split, P] of the whole flat vector for the last `forward(save=True)` (`FlatMLP.backward`'s
        contract): the combine's backward, the streams' weight slabs and input gradients, the feature join, the trunk's slabs
        -- all over the effective layout --, then `tsm_noisy_grad` onto the flat layout.  No forward may come between."""
        if self._saved_forward() is False:
            raise RuntimeError("RainbowNet.backward must follow its forward(save=True): a later forward recomposed the weights")
        z, training = self._saved
        R, Pe = z.shape[0], int(self.table.P_eff)
        n_split, slabs = self._slabs(R, n_split, slabs)
        eff_slabs = self._eff_slabs.get(n_split)
        if eff_slabs is None:
            eff_slabs = self._eff_slabs[n_split] = torch.empty(n_split, Pe, dtype=torch.float32, device=self.flat.device)
        d_out = d_out.reshape(R, self.dims[-1]).contiguous()
        if self.dueling:
            H = self.hidden_sizes[-1]
            d_q, d_v = ops.dueling_combine_backward(d_out, self.n_act, self.num_atoms)
            self.Q.backward(d_q, n_split, slabs=eff_slabs[:, self._parts[1][0]:], slab_stride=Pe)
            self.V.backward(d_v, n_split, slabs=eff_slabs[:, self._parts[2][0]:], slab_stride=Pe)
            d_z = ops.dueling_features_backward(z, self.Q.input_grad(d_q, 0, H), self.V.input_grad(d_v, 0, H))
        else:
            d_z = d_out
        self.trunk.backward(d_z, n_split, slabs=eff_slabs, slab_stride=Pe)
        return ops.noisy_grad(self.table, self.flat.data, eff_slabs, training, slabs=slabs)

    # ---- reference checkpoint compatibility ---------------------------------------------------------------------------
    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """`model.model.{2 i}`, `Q.model.{2 i}`, `V.model.{2 i}` (every MLP is Linear, activation, Linear, ...), each with
        `.mu_W` ... `.eps_q` or `.weight`, `.bias` (tests/golden/rainbow.npz, sd_*)."""
        stems = [f"{name}.model.{2 * i}" for name, c in zip(("model", "Q", "V"), self._chains) for i in range(len(c) - 1)]
        return [(f"{s}.{k}", t) for s, v in zip(stems, self.layer_views(flat)) for k, t in v.items()]


class BranchingNet(FlatNet):
    """The reference's `BranchingNet` (common.py:557-678, arXiv 1711.08946) on ONE flat f32 vector [common | value | branches].
    `common` (obs -> h_1 .. h_n) and `value` (h_n -> value_hidden -> 1) are `FlatMLP`s over slices of it (csrc/dense.hip); the K
    branches (h_n -> action_hidden -> A each) lie behind them in `EnsembleLinear`'s layout with E = K -- per layer weight
    [K, in, out], then bias [K, 1, out] -- and run as ONE grouped launch per layer (csrc/ensemble.hip).  The reference's common
    MLP ends in its activation (output_dim = 0): here its last layer stays linear and `tsm_dueling_features` applies the ReLU, so
    that `tsm_dueling_features_backward` can join the two streams' gradients behind it, as in `RainbowNet`.  The per-branch
    dueling combine is `tsm_bdqn_combine` (csrc/bdqn.hip).  Only no norm layer and ReLU are served.

    `forward(obs)` -> (logits [B, K, A], state).  `backward((d_adv, d_v))` takes the gradients w.r.t. the branches' raw outputs
    [K, B, A] and the value [B], with the combine's backward already folded in, as `ops.bdqn_head` returns them."""

    def __init__(self, *, state_shape, num_branches: int = 0, action_per_branch: int = 2, common_hidden_sizes=None,
                 value_hidden_sizes=None, action_hidden_sizes=None, norm_layer=None, norm_args=None, activation=nn.ReLU,
                 act_args=None, device: str | torch.device = "cuda", seed: int | None = None,
                 storage: torch.Tensor | None = None) -> None:
        super().__init__()
        for name, v in (("norm_layer", norm_layer), ("norm_args", norm_args), ("act_args", act_args)):
            if v is not None:
                raise NotImplementedError(f"BranchingNet: {name} = {v!r} is not served (no norm layer, plain ReLU)")
        if activation is not nn.ReLU and activation != "relu":
            raise NotImplementedError(f"BranchingNet: activation = {activation!r} is not served (ReLU only)")
        common_hidden_sizes = [int(h) for h in (common_hidden_sizes or [])]
        self.value_hidden_sizes = [int(h) for h in (value_hidden_sizes or [])]
        self.action_hidden_sizes = [int(h) for h in (action_hidden_sizes or [])]
        self.state_shape = state_shape
        K, A = self.num_branches, self.action_per_branch = int(num_branches), int(action_per_branch)
        ops.bdqn_check(K, A)
        H = common_hidden_sizes[-1]   # an empty list fails here, as in the reference (common.py:633)
        self.common_hidden_sizes = common_hidden_sizes
        D = int(np.prod(state_shape))
        self._chains = [[D, *common_hidden_sizes], [H, *self.value_hidden_sizes, 1], [H, *self.action_hidden_sizes, A]]
        self.branch_desc = ops.mlp_desc(self._chains[2], "relu")
        sizes = [ops.mlp_param_count(ops.mlp_desc(c, "relu")) for c in self._chains[:2]] + [ops.ens_mlp_param_count(self.branch_desc, K)]
        self.v_off, self.b_off = sizes[0], sizes[0] + sizes[1]
        self._branches = _GroupedLayers(self, self._chains[2], K, offset=self.b_off)
        self._b_offsets = self._branches.offsets
        assert self._branches.n_param == sizes[2]
        storage = self._claim(sum(sizes), storage, device)
        s = lambda k: None if seed is None else seed + k  # noqa: E731
        self.common = FlatMLP(self._chains[0], "relu", device=storage.device, seed=s(0), storage=storage[:self.v_off])
        self.value = FlatMLP(self._chains[1], "relu", device=storage.device, seed=s(1), storage=storage[self.v_off:self.b_off])
        self.dims = [D, K * A]   # what the policies ask of a Q-network: input width, outputs per row
        self.reset_branches(s(2))

    # ---- views ------------------------------------------------------------------------------------------------------------
    @property
    def branch_flat(self) -> torch.Tensor:
        return self.flat.data[self.b_off:]

    def branch_weight(self, i: int, flat: torch.Tensor | None = None) -> torch.Tensor:
        """Layer i of the branches: weight [K, in, out], a view of the flat vector (or of any vector of its layout)."""
        return self._branches.weight(i, flat)

    def branch_bias(self, i: int, flat: torch.Tensor | None = None) -> torch.Tensor:
        """Layer i of the branches: bias [K, 1, out]."""
        return self._branches.bias(i, flat)

    def reset_branches(self, seed: int | None = None) -> None:
        """torch nn.Linear default init of every branch layer: uniform +-1 / sqrt(in) for the weight and for the bias."""
        self._branches.reset(seed, lambda k: 1.0 / math.sqrt(k))

    # ---- forward / backward -------------------------------------------------------------------------------------------------
    def forward(self, obs, state=None, info=None, save: bool = True):
        """obs [..., D] -> (logits [B, K, A], state): trunk -> features -> value, K branches -> combine."""
        x = obs if isinstance(obs, torch.Tensor) else torch.as_tensor(np.asarray(obs, np.float32))
        x = x.to(self.flat.device, torch.float32).contiguous().reshape(-1, self.dims[0])
        z = FlatMLP.forward(self.common, x, save=save)
        f = ops.dueling_features(z)
        v = FlatMLP.forward(self.value, f, save=save)
        adv, acts = ops.ens_mlp_forward(self.branch_desc, self.num_branches, self.branch_flat, f)
        if save:
            self._saved = (z, f, acts)
        return ops.bdqn_combine(adv, v), state

    def backward(self, d_out, n_split: int = 0, slabs: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient slabs [n_split, P] of the whole flat vector for the last `forward(save=True)` (`FlatMLP.backward`'s
        contract), d_out = (d_adv, d_v): the branches' weight slabs and their branch-summed input gradient (members in order),
        the value stream's slabs and input gradient, the feature join, the trunk's slabs."""
        z, f, acts = self._saved_forward()
        d_adv, d_v = d_out
        B, P, H, K = z.shape[0], self.flat.numel(), self._chains[0][-1], self.num_branches
        n_split, slabs = self._slabs(B, n_split, slabs)
        d_adv =d_adv.reshape(K, B, self.action_per_branch).contiguous()
        d_v = d_v.reshape(B, 1).contiguous()
        ops.ens_mlp_backward(self.branch_desc, K, self.branch_flat, f, acts, d_adv, n_split, slabs=slabs[:, self.b_off:], slab_stride=P)
        d_fq = ops.ens_mlp_input_grad(self.branch_desc, K, self.branch_flat, f, acts, d_adv, 0, H)
        self.value.backward(d_v, n_split, slabs=slabs[:, self.v_off:], slab_stride=P)
        d_z = ops.dueling_features_backward(z, d_fq, self.value.input_grad(d_v, 0, H))
        self.common.backward(d_z, n_split, slabs=slabs, slab_stride=P)
        return slabs

    # ---- reference checkpoint compatibility ---------------------------------------------------------------------------
    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """[(key, view)] of `flat` (None: the net's own vector; else any vector of its layout, e.g. an Adam moment) in the
        reference module's `parameters()` order and shapes: `common.model.{2 i}`, `value.model.{2 i}`, then per branch
        `branches.{k}.model.{2 i}` -- `nn.Linear`'s [out, in], the transpose of the grouped layout's [in, out] slice."""
        flat = self._vector(flat)
        out = []
        for name, net, lo, hi in (("common", self.common, 0, self.v_off), ("value", self.value, self.v_off, self.b_off)):
            out += net.named_layers(ref_layer_keys(net.n_layers, "seq"), f"{name}.model.", flat[lo:hi])
        for k in range(self.num_branches):
            for i, (kw, kb) in enumerate(ref_layer_keys(self._branches.n_layers, "seq")):
                out += [(f"branches.{k}.model.{kw}", self.branch_weight(i, flat)[k].t()),
                        (f"branches.{k}.model.{kb}", self.branch_bias(i, flat)[k, 0])]
        return out


def _trunk_keys(ref_keys: dict | None, trunk: str, n_layers: int) -> list[tuple[str, str]]:
    """[(weight key, bias key)] of the "actor" / "critic" trunk: those of the modules the net was built from (`ref_keys`,
    `net_from_reference_modules`), else a DiscreteActor / DiscreteCritic over Net(hidden_sizes=[...])'s."""
    return (ref_keys or {}).get(trunk) or ref_layer_keys(n_layers, "head")


class DiscreteActorCritic(FlatNet):
    """Separate actor and critic MLP trunks, obs[D] -> H -> H -> (A logits | 1 value), flat parameters: actor then critic, each
    w0 b0 w1 b1 w2 b2 (the fused 64-wide kernels, csrc/mlp_fused.hip).  `ref_keys`: see `_trunk_keys`."""

    # a bare `FlatAdam` over this net has always listed ONE parameter, and tests/golden/flat_nets.npz pins that layout (PPO
    # lists its moments per reference parameter all the same: `FlatAdam(views=)`)
    split_optimizer_state = False

    def __init__(self, obs_dim: int, n_act: int, hidden: int = 64, device: str | torch.device = "cuda",
                 init: str = "orthogonal", seed: int | None = None, storage: torch.Tensor | None = None,
                 ref_keys: dict | None = None) -> None:
        super().__init__()
        self.obs_dim, self.n_act, self.hidden, self._ref_keys = int(obs_dim), int(n_act), int(hidden), ref_keys
        self._claim(ops.policy_param_count(self.obs_dim, self.hidden, self.n_act), storage, device)
        # padded LDS-layout copy of the parameters, refreshed by the Adam kernel (csrc/adam.hip) and by
        # sync_image(); the fused kernels stage it with straight 16-B copies
        self.image, self.image_map = ops.policy_image(self.obs_dim, self.hidden, self.n_act, device)
        # the orthogonal init seeds and draws from torch's GLOBAL generators; over given `storage` -- a twin, whose vector
        # `lagged_copy` fills -- nothing is drawn and no generator, host or device, is touched
        if storage is None:
            self.reset_parameters(init, seed)
        else:
            self.sync_image()

    def sync_image(self) -> None:
        ops.scatter_image(self.flat.data, self.image, self.image_map)

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """In ActorCritic.parameters() order with the key names `Algorithm.state_dict()` gives the reference's PPO over
        DiscreteActor/DiscreteCritic(Net(hidden_sizes=[H, H])): `policy.actor.<...>`, `critic.<...>`
        (algorithm_base.py:521-541; verified by tests/golden/checkpoint.npz)."""
        flat, o, out = self._vector(flat), 0, []
        D, H = self.obs_dim, self.hidden
        for trunk, prefix, n_out in (("actor", "policy.actor.", self.n_act), ("critic", "critic.", 1)):
            for (kw, kb), (n, k) in zip(_trunk_keys(self._ref_keys, trunk, 3), ((H, D), (H, H), (n_out, H))):
                out += [(prefix + kw, flat[o:o + n * k].view(n, k)), (prefix + kb, flat[o + n * k:o + n * k + n])]
                o += n * k + n
        return out

    def view(self, name: str) -> torch.Tensor:
        """`actor.w0`, `actor.b0`, ... `critic.b2`: that layer's weight or bias."""
        trunk, layer = name.split(".")
        return self.reference_named_views()[6 * ("actor", "critic").index(trunk) + 2 * int(layer[1]) + "wb".index(layer[0])][1]

    @torch.no_grad()
    def reset_parameters(self, init: str = "orthogonal", seed: int | None = None) -> None:
        """orthogonal weights + zero bias (the reference scripts' init, test/discrete/test_ppo_discrete.py:103-106)
        or torch's nn.Linear default (kaiming-uniform).  Seeded, every orthogonal weight re-seeds the global generator from a
        private one; `MLPActorCritic` seeds it once: two draws, and each class keeps its own."""
        gen = _generator(seed)
        views = [v for _, v in self.reference_named_views()]
        for W, b in zip(views[::2], views[1::2]):
            if init == "orthogonal":
                if gen is not None:
                    torch.manual_seed(int(torch.randint(0, 2**31 - 1, (1,), generator=gen)))
                W.copy_(nn.init.orthogonal_(torch.empty(W.shape)))
                b.zero_()
            else:
                bound = 1.0 / math.sqrt(W.shape[1])
                W.copy_(_uniform(W.shape, bound, gen))
                b.copy_(_uniform(b.shape, bound, gen))
        self.sync_image()

    def load_reference_state_dict(self, sd, prefix: str = "") -> None:
        super().load_reference_state_dict(sd, prefix)
        self.sync_image()

    @torch.no_grad()
    def load_layers(self, actor, critic) -> None:
        """actor / critic: [(W, b)] * 3 (numpy or tensors) in torch nn.Linear layout."""
        for (_, v), t in zip(self.reference_named_views(), [t for layer in (*actor, *critic) for t in layer]):
            v.copy_(torch.as_tensor(np.asarray(t)).to(v.device, torch.float32))
        self.sync_image()


class MLPActorCritic(FlatNet):
    """Actor and critic MLPs of ARBITRARY widths under one flat parameter vector (`ActorCritic(actor, critic)`,
    common.py:461-474: one optimizer, one global gradient-norm clip).  Layout = actor parameters then critic parameters,
    each in torch `parameters()` order; `actor` / `critic` are `FlatMLP` views into it (csrc/dense.hip).  Use with
    `tianshou_marl_amd.algorithm.ppo_generic.GenericPPO` when the 64-wide fused kernels do not apply (hidden sizes
    other than 64, more layers, tanh, or a centralized critic: `critic_obs_dim = n_agent * obs_dim`)."""

    split_optimizer_state = False
    image = image_map = None  # no LDS image: the dense kernels stream the weights

    def __init__(self, obs_dim: int, n_act: int, hidden_sizes=(128, 128), act: str = "relu",
                 critic_obs_dim: int | None = None, device: str | torch.device = "cuda", seed: int | None = None,
                 init: str = "orthogonal", storage: torch.Tensor | None = None, ref_keys: dict | None = None) -> None:
        super().__init__()
        self.obs_dim, self.n_act, self.hidden, self._ref_keys = int(obs_dim), int(n_act), int(hidden_sizes[0]), ref_keys
        self.critic_obs_dim = int(critic_obs_dim or obs_dim)
        dims_a = [self.obs_dim, *hidden_sizes, self.n_act]
        dims_c = [self.critic_obs_dim, *hidden_sizes, 1]
        na = ops.mlp_param_count(ops.mlp_desc(dims_a, act))
        nc = ops.mlp_param_count(ops.mlp_desc(dims_c, act))
        flat = self._claim(na + nc, storage, device)
        self.n_actor, self.n_critic = na, nc
        # the trunks' own constructors draw nn.Linear's init from the global generator, and the init proper seeds it; over
        # given `storage` (a twin, as in `DiscreteActorCritic`) the trunks draw from a private one and the init is left out
        trunk_seed = None if storage is None else 0
        self.actor = FlatMLP(dims_a, act, device=device, seed=trunk_seed, storage=flat[:na])
        self.critic = FlatMLP(dims_c, act, device=device, seed=trunk_seed, storage=flat[na:])
        if storage is None:
            self.reset_parameters(init, seed)

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """As DiscreteActorCritic.reference_named_views, for Net(hidden_sizes=[...]) of any depth: hidden layer i is
        `preprocess.model.model.{2 i}` (Linear, activation, Linear, ...), the output layer `last.model.0`."""
        flat, na = self._vector(flat), self.n_actor
        return [kv for name, net, prefix, part in (("actor", self.actor, "policy.actor.", flat[:na]),
                                                   ("critic", self.critic, "critic.", flat[na:]))
                for kv in net.named_layers(_trunk_keys(self._ref_keys, name, net.n_layers), prefix, part)]

    @torch.no_grad()
    def reset_parameters(self, init: str = "orthogonal", seed: int | None = None) -> None:
        """orthogonal weights + zero bias (the reference scripts' init) or nn.Linear's default."""
        if seed is not None:
            torch.manual_seed(seed)
        for net in (self.actor, self.critic):
            if init != "orthogonal":
                net.reset_parameters(seed)
                continue
            for i in range(net.n_layers):
                w = torch.empty(net.weight(i).shape)
                nn.init.orthogonal_(w)
                net.weight(i).copy_(w)
                net.bias(i).zero_()


def _one_parameter(flat: torch.Tensor) -> list[torch.Tensor]:
    return [flat]


class FlatAdam:
    """torch.optim.Adam semantics (algorithm_base.py:485-498 wraps it) on one flat parameter vector, executed by
    `tsm_adam_step` (slab reduction + optional grad-norm clip + Adam in one launch).  Stands where
    `optim.Adam(module.parameters(), lr=...)` stands in the reference's CTDE constructors (ctde.py:36-37)."""

    def __init__(self, module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: float | None = None, coef64: bool = False, views=None) -> None:
        self.coef64 = bool(coef64)  # `step` runs tsm_adam_step_coef64: torch's own f32 coefficients 1 - beta
        self.param = module.flat.data if hasattr(module, "flat") else module
        # a vector of the parameter's layout (a moment) -> the parameters it holds, in the vector's order: the net's own
        # statement; a bare vector, or a module that states none, is one parameter.  `views`: the owner's statement instead
        # (PPO: per reference parameter, also where the net's own optimizer checkpoints list the vector whole)
        self._views = views or getattr(module, "param_views", _one_parameter)
        self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.exp_avg = torch.zeros_like(self.param)
        self.exp_avg_sq = torch.zeros_like(self.param)
        self.step_count = 0
        self.work = torch.zeros(ops.call("tsm_adam_work_elems", self.param.numel()), dtype=torch.float32,
                                 device=self.param.device)

    def zero_grad(self) -> None:  # gradients are produced fresh per step as slabs; nothing accumulates
        return None

    def step(self, grad_slabs: torch.Tensor) -> None:
        self.step_count += 1
        ops.adam_step(self.param, grad_slabs, self.exp_avg, self.exp_avg_sq, self.step_count, lr=self.lr,
                      betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, max_grad_norm=self.max_grad_norm,
                      work=self.work, coef64=self.coef64)

    def step_segs(self, segs: list, step_dev: torch.Tensor | None = None) -> None:
        """`step` for gradients that arrive as several slab arrays (ops.adam_step_segs: segments tiling the vector, each
        optionally scaled by a device scalar).  step_dev: device-resident step count (captured graphs)."""
        if step_dev is None:
            self.step_count += 1
        ops.adam_step_segs(self.param, segs, self.exp_avg, self.exp_avg_sq, self.step_count if step_dev is None else 1,
                           lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                           max_grad_norm=self.max_grad_norm, work=self.work, step_dev=step_dev)

    def _shapes(self) -> list[tuple[int, ...]]:
        return [tuple(v.shape) for v in self._views(self.exp_avg)]

    def state_dict(self) -> dict:
        """torch.optim.Adam.state_dict() layout (per-parameter `state`, one `param_groups` entry), parameters in the
        module's `parameters()` order -- what `optim_actor.state_dict()` gives in the reference (ctde.py:36-37)."""
        state = {}
        views = list(zip(self._views(self.exp_avg), self._views(self.exp_avg_sq)))
        if self.step_count > 0:
            for i, (m, v) in enumerate(views):
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": m.contiguous().clone(),
                            "exp_avg_sq": v.contiguous().clone()}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "decoupled_weight_decay": False, "params": list(range(len(views)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: dict) -> None:
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        step = 0
        for i, (m, v) in enumerate(zip(self._views(self.exp_avg), self._views(self.exp_avg_sq))):
            e = sd["state"].get(i, sd["state"].get(str(i)))
            if e is not None:
                m.copy_(torch.as_tensor(e["exp_avg"]).reshape(m.shape))
                v.copy_(torch.as_tensor(e["exp_avg_sq"]).reshape(v.shape))
                step = int(float(e["step"]))
        g = sd["param_groups"][0]
        self.step_count, self.lr = step, float(g["lr"])
        self.betas, self.eps, self.weight_decay = tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"])


# ---- lagged copies and joint parameter vectors -------------------------------------------------------------------------------
def lagged_copy(net, storage: torch.Tensor | None = None):
    """A twin of `net` over storage of its own (None: a clone of the flat vector), holding the same weights: a lagged or
    target network, or a second critic.  The twin's constructor draws its init from a private generator (`clone_over` gives a
    seed) and the copy overwrites that draw, so the global torch RNG is not drawn from -- as the reference's deepcopy draws
    nothing, and a seeded script's later torch.randint / nn.Linear init stays the reference's."""
    if storage is None:
        storage = net.flat.data.clone()
    twin = net.clone_over(storage)
    storage.copy_(net.flat.data)
    twin.sync_image()
    return twin


def join_nets(nets, device) -> tuple[torch.Tensor, list[int]]:
    """ONE flat parameter vector [net_0 | net_1 | ...] on `device`: every net's parameters move into its slice (`rebind`) and
    are viewed there.  -> (flat, offsets): net k occupies flat[offsets[k]:offsets[k + 1]]."""
    offsets = np.concatenate([[0], np.cumsum([n.flat.numel() for n in nets])]).astype(np.int64).tolist()
    flat = torch.zeros(offsets[-1], dtype=torch.float32, device=device)
    for n, o, e in zip(nets, offsets, offsets[1:]):
        n.rebind(flat[o:e])
    return flat, offsets


def lagged_twins(nets, flat: torch.Tensor, offsets) -> tuple[torch.Tensor, list]:
    """The targets of the nets that `join_nets` joined: -> (target_flat, a copy of `flat`; a twin of every net over its slice
    of it).  One copy fills all of them, RNG-neutral as `lagged_copy`."""
    target_flat = flat.clone()
    twins = [n.clone_over(target_flat[o:e]) for n, o, e in zip(nets, offsets, offsets[1:])]
    target_flat.copy_(flat)
    for t in twins:
        t.sync_image()
    return target_flat, twins


# ---- the intrinsic curiosity module (utils/net/discrete.py:378-429) -------------------------------------------------------------
class IntrinsicCuriosityModule(FlatNet):
    """discrete.py:378-429: a feature net, a forward model [phi1 | one_hot(act)] -> phi2_hat and an inverse model
    [phi1 | phi2] -> act_hat, as three `FlatMLP`s on ONE flat vector [feature_net | forward_model | inverse_model] (the
    reference's `parameters()` order).  `feature_net`: a `FlatMLP` whose last width is `feature_dim`; its parameters move into
    the joint vector.  `hidden_sizes`: of the two models (ReLU, as the reference's `MLP`).

    The feature net runs once over 2R interleaved rows (obs of row r at 2r, obs_next at 2r + 1), so its output viewed as
    [R, 2 feature_dim] is the inverse model's input without a copy.  `forward` keeps what `head` and `backward` need: the pair
    replaces autograd for this module (csrc/icm.hip, csrc/dense.hip)."""

    def __init__(self, *, feature_net: FlatMLP, feature_dim: int, action_dim: int, hidden_sizes=()) -> None:
        super().__init__()
        if not isinstance(feature_net, FlatMLP) or type(feature_net).forward is not FlatMLP.forward:
            raise TypeError(f"IntrinsicCuriosityModule needs a FlatMLP feature net: the update runs in HIP, there is no autograd "
                            f"fallback (got {type(feature_net).__name__})")
        F, A = int(feature_dim), int(action_dim)
        if feature_net.dims[-1] != F:
            raise ValueError(f"IntrinsicCuriosityModule: the feature net has {feature_net.dims[-1]} outputs, feature_dim is {F}")
        ops.icm_check(F, A)
        dev = feature_net.flat.device
        self.feature_dim, self.action_dim = F, A
        self.feature_net = feature_net
        self.forward_model = FlatMLP([F + A, *hidden_sizes, F], "relu", device=dev)
        self.inverse_model = FlatMLP([2 * F, *hidden_sizes, A], "relu", device=dev)
        flat, self._offs = join_nets(self.nets, dev)
        self._claim(flat.numel(), flat, dev)

    @property
    def nets(self) -> list[FlatMLP]:
        return [self.feature_net, self.forward_model, self.inverse_model]

    @property
    def head(self):
        """What the last `forward(save=True)` left for `backward`: ops.icm_head's outputs (None: nothing)."""
        return self._saved

    def forward(self, s1, act, s2, save: bool = True, **kwargs):
        """s1, s2 [R, D], act [R] -> (mse_loss f32 [R], act_hat f32 [R, action_dim]) in HBM (discrete.py:411-429).  kwargs: the
        loss weights and the reward shaping of `forward_rows`."""
        dev = self.flat.device
        s1 = torch.as_tensor(s1).to(dev, torch.float32)
        s2 = torch.as_tensor(s2).to(dev, torch.float32)
        D = self.feature_net.dims[0]
        x = torch.empty(s1.numel() // D, 2, D, dtype=torch.float32, device=dev)
        x[:, 0].copy_(s1.reshape(-1, D))
        x[:, 1].copy_(s2.reshape(-1, D))
        return self.forward_rows(x.view(-1, D), act, save=save, **kwargs)

    def forward_rows(self, x: torch.Tensor, act, save: bool = True, rew_io=None, ids=None, reward_scale: float = 0.0,
                     forward_loss_weight: float | None = None, lr_scale: float | None = None):
        """`forward` on rows that are interleaved already: x [2R, D].  With `save`, the head's gradients for the given
        `forward_loss_weight` / `lr_scale` are kept for `backward`, so both must be given (`backward` returns the gradient of
        the loss they define); `rew_io` / `ids` / `reward_scale`: the in-place reward shaping of `ops.icm_head`."""
        if save and (forward_loss_weight is None or lr_scale is None):
            raise ValueError("IntrinsicCuriosityModule.forward(save=True) needs forward_loss_weight= and lr_scale=: the head forms "
                             "the gradients that backward() returns; pass save=False for the outputs alone")
        forward_loss_weight, lr_scale = float(forward_loss_weight or 0.0), float(lr_scale or 0.0)
        dev = self.flat.device
        act = torch.as_tensor(act).to(dev, torch.int64).reshape(-1)
        F, A = self.feature_dim, self.action_dim
        R = act.numel()
        if x.shape[0] != 2 * R:
            raise ValueError(f"IntrinsicCuriosityModule: {x.shape[0]} rows of obs / obs_next for {R} actions")
        phi = self.feature_net.forward(x, save=save)                       # [2R, F]
        phi2_hat = self.forward_model.forward(ops.icm_rows(phi, act, A), save=save)
        act_hat = self.inverse_model.forward(phi.view(R, 2 * F), save=save)
        head = ops.icm_head(phi2_hat, phi, act_hat, act, reward_scale, forward_loss_weight, lr_scale, rew_io=rew_io, ids=ids)
        self._saved = head if save else None
        return head["mse"], act_hat

    def backward(self, n_split: int = 0, slabs: torch.Tensor | None = None) -> torch.Tensor:
        """Gradient slabs [n_split, n_param] of the whole vector for the last `forward(save=True)`: the two models' backwards,
        their input gradients, `ops.icm_join_grad`, one feature-net backward on the 2R rows."""
        h, F = self._saved_forward(), self.feature_dim
        R, P = h["mse"].numel(), self.flat.numel()
        n_split, slabs = self._slabs(R, n_split, slabs)
        o = self._offs
        self.forward_model.backward(h["d_phi2_hat"], n_split, slabs=slabs[:, o[1]:], slab_stride=P)
        self.inverse_model.backward(h["d_act_hat"], n_split, slabs=slabs[:, o[2]:], slab_stride=P)
        g_fwd = self.forward_model.input_grad(h["d_phi2_hat"], 0, F)
        g_inv = self.inverse_model.input_grad(h["d_act_hat"], 0, 2 * F)
        d_phi = ops.icm_join_grad(g_fwd, g_inv, h["d_phi2_fwd"])
        self.feature_net.backward(d_phi, n_split, slabs=slabs, slab_stride=P)
        return slabs

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        """Three `MLP`s: `ref_layer_keys`' "seq" under `<name>.model.`."""
        flat, o = self._vector(flat), self._offs
        return [kv for k, (name, m) in enumerate(zip(("feature_net", "forward_model", "inverse_model"), self.nets))
                for kv in m.named_layers(ref_layer_keys(m.n_layers, "seq"), f"{name}.model.", flat[o[k]:o[k + 1]])]


class RunningMeanStd:
    """tianshou.utils.statistics.RunningMeanStd (statistics.py:68-114), scalar statistics, host f64.
    The batch moments come from a device reduction; only three scalars live on the host."""

    def __init__(self, mean: float = 0.0, std: float = 1.0, clip_max: float | None = 10.0,
                 epsilon: float = float(np.finfo(np.float32).eps)) -> None:
        self.mean, self.var = mean, std  # NB: the reference stores `std` into var (statistics.py:92)
        self.clip_max, self.count, self.eps = clip_max, 0, epsilon

    def update_from_moments(self, batch_mean: float, batch_var: float, batch_count: int) -> None:
        delta = batch_mean - self.mean
        total = self.count + batch_count
        new_mean = self.mean + delta * batch_count / total
        m_2 = self.var * self.count + batch_var * batch_count + delta**2 * self.count * batch_count / total
        self.mean, self.var, self.count = new_mean, m_2 / total, total

    def update(self, x) -> None:
        if isinstance(x, torch.Tensor):
            xd = x.double()
            self.update_from_moments(float(xd.mean()), float(xd.var(unbiased=False)), x.numel())
        else:
            a = np.asarray(x, np.float64)
            self.update_from_moments(float(a.mean()), float(a.var()), a.size)


class DeviceRunningMeanStd(RunningMeanStd):
    """The same statistics with their state in HBM: `dev` = f64 {mean, var, count}.  The GAE kernel reads the scale
    sqrt(var + eps) from it and `tsm_rms_update` merges a batch of unnormalised returns into it (a2c.py:132-146), so
    `return_scaling` needs no host round trip and survives hipGraph replays.  `mean` / `var` / `count` read (and
    write) the device state; reading synchronises."""

    def __init__(self, device, mean: float = 0.0, std: float = 1.0, clip_max: float | None = 10.0,
                 epsilon: float = float(np.finfo(np.float32).eps)) -> None:
        self.dev = torch.tensor([mean, std, 0.0], dtype=torch.float64, device=device)
        self.clip_max, self.eps = clip_max, epsilon

    def _get(self, i: int) -> float:
        return float(self.dev[i].item())

    mean = property(lambda s: s._get(0), lambda s, v: s.dev[0:1].fill_(float(v)))
    var = property(lambda s: s._get(1), lambda s, v: s.dev[1:2].fill_(float(v)))
    count = property(lambda s: int(s._get(2)), lambda s, v: s.dev[2:3].fill_(float(v)))

    def update_scaled_returns(self, returns: torch.Tensor, rms_eps: float, ids: torch.Tensor | None = None) -> None:
        """update(returns * sqrt(var + rms_eps)) entirely on device (a2c.py:144-146)."""
        ops.rms_update(returns, self.dev, rms_eps, ids=ids)


def net_from_reference_modules(policy, critic, device="cuda"):
    """Build the flat HBM network from reference-shaped torch modules (`utils/ref_nets.py` mirrors or the reference's
    own `DiscreteActorPolicy` / `DiscreteCritic`): parameters are copied once, the key names of the modules'
    `state_dict()` are remembered for checkpoints.  64-64 ReLU nets on observations of at most 64 floats run on the
    fused kernels (DiscreteActorCritic); everything else on the general MLP kernels (MLPActorCritic).
    critic=None (Reinforce): the fused layout always carries a critic trunk; it stays untouched."""
    from .ref_nets import activation_of, linear_layers, reference_key_names

    cached = getattr(policy, "_tsm_net", None)
    if cached is not None and cached[0] is critic and str(cached[1].flat.device).startswith(str(device).split(":")[0]):
        return cached[1]
    actor_mod = getattr(policy, "actor", policy)
    la = linear_layers(actor_mod)
    act = activation_of(actor_mod)
    obs_dim, n_act = la[0][0].shape[1], la[-1][0].shape[0]
    hidden = [w.shape[0] for w, _ in la[:-1]]
    if critic is not None:
        lc = linear_layers(critic)
        if activation_of(critic) != act and len(lc) > 1:
            raise ValueError("actor and critic must use the same activation")
        if [w.shape[0] for w, _ in lc[:-1]] != hidden or lc[-1][0].shape[0] != 1:
            raise ValueError("actor and critic must have the same hidden sizes and the critic a single output")
        critic_obs = lc[0][0].shape[1]
    else:
        lc, critic_obs = None, obs_dim
    # (no critic: both trunks under the default names)
    ref_keys = {"actor": reference_key_names(actor_mod), "critic": reference_key_names(critic)} if critic is not None else None
    if len(la) == 3 and hidden == [64, 64] and obs_dim <= 64 and n_act <= 16 and act == "relu" and critic_obs == obs_dim:
        net = DiscreteActorCritic(obs_dim, n_act, 64, device=device, ref_keys=ref_keys)
        if lc is None:
            lc = [(np.zeros_like(net.view(f"critic.w{i}").cpu().numpy()), np.zeros_like(net.view(f"critic.b{i}").cpu().numpy()))
                  for i in range(3)]
        net.load_layers(la, lc)
    else:
        if lc is None:
            raise ValueError("Reinforce without a critic runs on the fused 64-64 layout only")
        net = MLPActorCritic(obs_dim, n_act, tuple(hidden), act=act, critic_obs_dim=critic_obs, device=device, ref_keys=ref_keys)
        net.actor.load_layers(la)
        net.critic.load_layers(lc)
    try:
        policy._tsm_net = (critic, net)
    except Exception:  # noqa: BLE001  (objects without attribute assignment: no cache)
        pass
    return net
