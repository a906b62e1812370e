"""Coordinate networks with the reference's class surface, computed by the gfx950 kernels.

Mirrors reference `models.py`: `BaseMLP` (models.py:20-95), `Sine` (:108-114), `SirenLayer`
(:117-156), `SirenNet` (:160-233), `Modulator` / `ModulatedSirenNet` (:236-322), `HashMLP` (:658-754): same constructor arguments,
`PsfSirenNet` (:397-539): same constructor arguments,
`RffNet` (:542-584): same constructor arguments,
`RealGaborLayer` (:757-788) / `GaborNet` (:836-885): same constructor arguments (the complex layer is refused),
`forward(x)`, `training_step`, `predict_step`, `configure_optimizers`, same state-dict keys.
Known defects of the reference are resolved to the INTENDED semantics:
  Q1  HashMLP.forward applies the decoder blocks in sequence (the reference calls a ModuleList);
  Q2  BaseMLP.forward runs `self.layers(x)` (the reference recurses into itself);
  Q3  HashMLP does not build BaseMLP's unused default `layers` stack; checkpoints that carry
      those dead `layers.*` keys still load;
  Q13 PsfSirenNet(coordinates_spacing=None) raises ValueError("No PSF spacing defined") (the reference's
      `coordinates_spacing if not None else ValueError(...)` never raises, and its constructor then fails
      inside torch.linspace).
Every Linear(+activation) is one f32-MFMA kernel (csrc/linear.hip); there is no CPU path.
"""
import math
from typing import Tuple

import torch
import torch.nn as nn

from . import encoding, ops, optim

try:  # pragma: no cover - pytorch_lightning is optional (absent on the MI355X image)
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    class _Base(nn.Module):
        """The four LightningModule protocol methods the reference relies on."""

        @property
        def device(self):
            p = next(self.parameters(), None)
            return p.device if p is not None else torch.device("cpu")

        def log(self, name, value, *args, **kwargs):
            self._last_logged = {name: value}


def mse_loss(target: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
    """`F.mse_loss(y, y_pred)` as called at reference models.py:64 (target first), computed
    by the fused loss kernel; differentiable w.r.t. `pred`."""
    return ops.MSELossFunction.apply(pred, target)


def exists(val):
    return val is not None


def _activation_code(module_or_cls):
    """Map an activation module/class to a fused epilogue, or None if it must run unfused."""
    m = module_or_cls() if isinstance(module_or_cls, type) else module_or_cls
    if isinstance(m, nn.ReLU):
        return ops.ACT_RELU, 1.0
    if isinstance(m, nn.GELU) and getattr(m, "approximate", "none") == "none":
        return ops.ACT_GELU, 1.0
    if isinstance(m, nn.Identity):
        return ops.ACT_IDENTITY, 1.0
    if isinstance(m, Sine):
        return ops.ACT_SINE, float(m.w0)
    return None


class _Fused(nn.Module):
    """Placeholder kept where the reference has a separate activation module, so that
    Sequential indices (and state-dict keys) match; the math is fused into the Linear."""

    def __init__(self, name):
        super().__init__()
        self.name = name

    def forward(self, x):
        return x

    def extra_repr(self):
        return f"{self.name} (fused into the preceding Linear)"


class FusedLinear(nn.Linear):
    """nn.Linear whose forward is `act(w0 * (x W^T + b))` in one MFMA kernel."""

    def __init__(self, in_features, out_features, bias=True, activation=ops.ACT_IDENTITY,
                 w0=1.0):
        super().__init__(in_features, out_features, bias=bias)
        self.activation_code, self.w0 = activation, w0

    def forward(self, x):
        return ops.linear_act(x, self.weight, self.bias, self.activation_code, self.w0)


class BaseMLP(_Base):
    """Fully connected network, base class of the other models (reference models.py:20-95).
    Note the activation after the LAST Linear too (models.py:46-56)."""

    def __init__(self, dim_in: int = 2, dim_out: int = 1, dim_hidden: int = 128,
                 n_layers: int = 8, activation=nn.ReLU, criterion=mse_loss, lr: float = 1e-4,
                 *args, **kwargs) -> None:
        super().__init__()
        self.dim_in = dim_in
        self.dim_hidden = dim_hidden
        self.dim_out = dim_out
        self.n_layers = n_layers
        self.activation = activation
        self.criterion = criterion
        self.lr = lr
        if kwargs.pop("_build_layers", True):
            self.layers = self._make_stack(dim_in, dim_hidden, dim_out, n_layers, activation,
                                           final_activation=True)

    @staticmethod
    def _make_stack(dim_in, dim_hidden, dim_out, n_layers, activation, final_activation):
        code = _activation_code(activation)
        mods = []
        for i in range(n_layers):
            last = i == n_layers - 1
            fan_in = dim_in if i == 0 else dim_hidden
            fan_out = dim_out if last else dim_hidden
            act_here = final_activation or not last
            if act_here and code is not None:
                mods += [FusedLinear(fan_in, fan_out, activation=code[0], w0=code[1]),
                         _Fused(activation.__name__ if isinstance(activation, type)
                                else type(activation).__name__)]
            else:
                mods.append(FusedLinear(fan_in, fan_out))
                if act_here:
                    mods.append(activation())  # unfused torch module (not on the hot path)
        return nn.Sequential(*mods)

    def forward(self, x):
        return self.layers(x)

    def training_step(self, batch, batch_idx):
        x, y = batch
        y_pred = self.forward(x)
        loss = self.criterion(y, y_pred)
        self.log("train_loss", loss)
        return loss

    def configure_optimizers(self):
        self.optimizer = optim.Adam(self.parameters(), lr=self.lr)
        return self.optimizer

    def predict_step(self, batch, batch_idx):
        x, y = batch
        return self(x)

    def forward_with_gradient(self, x) -> Tuple[torch.Tensor, torch.Tensor]:
        """(y (n, 1), dydx (n, dim_in)), both detached: the prediction and its gradient with respect to the
        coordinates, dydx[i, d] = dy[i] / dx[i, d].  The generic body: autograd through the model's own `forward`
        (every op returns the gradient of its input; HashMLP through the hash grid's input backward).  The
        parameters gain no `.grad`."""
        if self.dim_out != 1:
            raise ValueError(f"forward_with_gradient needs dim_out == 1 (got {self.dim_out}): the gradient of one "
                             "output with respect to the coordinates")
        with torch.enable_grad():
            xg = x.detach().clone().requires_grad_(True)
            y = self.forward(xg)
            dydx, = torch.autograd.grad(y.sum(), xg)
        return y.detach(), dydx.detach()

    def set_parameters(self, theta):
        """Copy a sequence of tensors into the parameters, in state-dict order
        (reference models.py:87-96)."""
        sd = self.state_dict()
        for key, value in zip(sd, theta):
            sd[key] = value.data
        self.load_state_dict(sd)


class Sine(nn.Module):
    def __init__(self, w0=30.0):
        super().__init__()
        self.w0 = w0

    def forward(self, x):  # only reached when used outside a SirenLayer
        w = torch.eye(x.shape[-1], device=x.device)
        return ops.linear_act(x, w, None, ops.ACT_SINE, self.w0)


class SirenLayer(nn.Module):
    """sin(w0 (x W^T + b)) (reference models.py:117-156), one fused kernel."""

    def __init__(self, dim_in: int, dim_out: int = 1, w0: float = 30.0, sigma: float = 6.0,
                 is_first: bool = False, use_bias: bool = True, activation=None):
        super().__init__()
        self.dim_in = dim_in
        self.is_first = is_first
        weight = torch.zeros(dim_out, dim_in)
        bias = torch.zeros(dim_out) if use_bias else None
        self.init_(weight, bias, sigma=sigma, w0=w0)
        self.weight = nn.Parameter(weight)
        self.bias = nn.Parameter(bias) if use_bias else None
        self.activation = Sine(w0) if activation is None else activation
        self._code = _activation_code(self.activation)

    def init_(self, weight, bias, sigma, w0):
        # reference models.py:144-151
        bound = (1 / self.dim_in) if self.is_first else (math.sqrt(sigma / self.dim_in) / w0)
        weight.uniform_(-bound, bound)
        if exists(bias):
            bias.uniform_(-bound, bound)

    def forward(self, x):
        if self._code is not None:
            return ops.linear_act(x, self.weight, self.bias, self._code[0], self._code[1])
        return self.activation(ops.linear_act(x, self.weight, self.bias))


class SirenNet(BaseMLP):
    """SIREN (reference models.py:160-233)."""

    def __init__(self, dim_in: int = 3, dim_hidden: int = 64, dim_out: int = 1,
                 n_layers: int = 4, w0: float = 30.0, w0_initial: float = 30.0,
                 sigma: float = 6.0, use_bias: bool = True, final_activation=None,
                 lr: float = 1e-4):
        super().__init__(dim_in=dim_in, dim_out=dim_out, dim_hidden=dim_hidden,
                         n_layers=n_layers, lr=lr, _build_layers=False)
        self.sigma = sigma
        self.losses = []
        self.w0, self.w0_initial = w0, w0_initial
        self.layers = nn.ModuleList([])
        for ind in range(n_layers):
            first = ind == 0
            self.layers.append(SirenLayer(dim_in=dim_in if first else dim_hidden,
                                          dim_out=dim_hidden,
                                          w0=w0_initial if first else w0, sigma=sigma,
                                          use_bias=use_bias, is_first=first))
        final_activation = nn.Identity() if not exists(final_activation) else final_activation
        self.last_layer = SirenLayer(dim_in=dim_hidden, dim_out=dim_out, w0=w0, sigma=sigma,
                                     use_bias=use_bias, activation=final_activation)

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return self.last_layer(x)

    def _gradient_plan(self, x):
        """Arguments of the fused gradient kernel (csrc/siren_gradient.hip), or None where the generic body serves:
        the plain chain only -- sine layers with one w0 behind the first, an identity head, biases everywhere, a
        shape the kernel takes -- and a tensor on the GPU."""
        ls = list(self.layers) + [self.last_layer]
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or any(l.bias is None for l in ls):
            return None
        if any(not isinstance(l.activation, Sine) for l in ls[:-1]) or not isinstance(ls[-1].activation, nn.Identity):
            return None
        if len({float(l.activation.w0) for l in ls[1:-1]}) > 1:
            return None
        hidden, dim_in = ls[0].weight.shape
        if x.shape[1] != dim_in or any(l.weight.shape != (hidden, hidden) for l in ls[1:-1]) \
                or ls[-1].weight.shape != (1, hidden):
            return None
        if not ops.siren_gradient_supported(dim_in, hidden, len(ls) - 1, self.dim_out):
            return None
        w0_first = float(ls[0].activation.w0)
        return dict(weights=[l.weight.detach() for l in ls], biases=[l.bias.detach() for l in ls],
                    w0_first=w0_first, w0=float(ls[1].activation.w0) if len(ls) > 2 else w0_first)

    def forward_with_gradient(self, x) -> Tuple[torch.Tensor, torch.Tensor]:
        """As BaseMLP.forward_with_gradient; the plain chain on the GPU runs ONE kernel that carries the value and
        the tangents of a point through the layers together (ops.siren_gradient), everything else the generic
        body."""
        if self.dim_out != 1:
            raise ValueError(f"forward_with_gradient needs dim_out == 1 (got {self.dim_out})")
        plan = self._gradient_plan(x)
        if plan is None:
            return super().forward_with_gradient(x)
        with torch.no_grad():
            return ops.siren_gradient(x.detach(), plan["weights"], plan["biases"], plan["w0_first"], plan["w0"])


def cast_tuple(val, repeat=1):
    return val if isinstance(val, tuple) else ((val,) * repeat)


class Modulator(nn.Module):
    """ReLU modulator of 'Modulated periodic activations' (reference models.py:236-260): layer
    i sees cat(hidden_{i-1}, z); returns every hidden state.  Each Linear+ReLU is one fused
    kernel; state-dict keys `layers.{i}.0.weight/bias` as in the reference."""

    def __init__(self, dim_in, dim_hidden, n_layers):
        super().__init__()
        self.layers = nn.ModuleList([])
        for ind in range(n_layers):
            dim = dim_in if ind == 0 else (dim_hidden + dim_in)
            self.layers.append(nn.Sequential(
                FusedLinear(dim, dim_hidden, activation=ops.ACT_RELU), _Fused("ReLU")))

    def forward(self, z):
        x = z
        hiddens = []
        for layer in self.layers:
            x = layer(x)
            hiddens.append(x)
            x = torch.cat((x, z), dim=1)
        return tuple(hiddens)


class ModulatedSirenNet(SirenNet):
    """SIREN whose hidden layers are multiplied elementwise by a modulator's hidden states
    (reference models.py:263-322).  Like the reference, the class also carries the default
    SirenNet stack its base constructor builds (`layers.*`, `last_layer.*`: unused by
    forward, present in the state dict)."""

    def __init__(self, dim_in: int = 3, dim_hidden: int = 64, dim_out: int = 1,
                 n_layers: int = 4, w0: float = 30.0, w0_initial: float = 30.0,
                 sigma: float = 6.0, use_bias: bool = True, final_activation=None,
                 lr: float = 1e-4):
        super().__init__()
        self.dim_in = dim_in
        self.dim_hidden = dim_hidden
        self.dim_out = dim_out
        self.n_layers = n_layers
        self.w0 = w0
        self.w0_initial = w0_initial
        self.sigma = sigma
        self.use_bias = use_bias
        self.final_activation = final_activation
        self.lr = lr
        self.losses = []
        self.modulator = Modulator(dim_in=dim_in, dim_hidden=dim_hidden, n_layers=n_layers)
        self.siren = SirenNet(dim_in=dim_in, dim_hidden=dim_hidden, dim_out=dim_out,
                              n_layers=n_layers, w0=w0, w0_initial=w0_initial, sigma=sigma,
                              use_bias=use_bias, final_activation=final_activation, lr=lr)

    def forward(self, x):
        mods = cast_tuple(self.modulator(x), self.n_layers)
        for layer, mod in zip(self.siren.layers, mods):
            x = ops.modulate(layer(x), mod)
        return self.siren.last_layer(x)

    def _gradient_plan(self, x):
        """Arguments of the fused modulated gradient kernel (csrc/modsiren_gradient.hip), or None where the generic
        body serves: both stacks as the kernel computes them -- sine layers with one w0 behind the first, an identity
        head, biases everywhere, a shape the kernel takes (dim_in <= 3) -- and a float32 (n, dim_in) tensor on the
        GPU."""
        sn = self.siren
        ls = list(sn.layers) + [sn.last_layer]
        mods = [seq[0] for seq in self.modulator.layers]
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or any(l.bias is None for l in ls + mods):
            return None
        if any(not isinstance(l.activation, Sine) for l in ls[:-1]) or not isinstance(ls[-1].activation, nn.Identity):
            return None
        if len({float(l.activation.w0) for l in ls[1:-1]}) > 1:
            return None
        hidden, dim_in = ls[0].weight.shape
        if x.shape[1] != dim_in or len(mods) != len(ls) - 1 or ls[-1].weight.shape != (1, hidden) \
                or any(l.weight.shape != (hidden, hidden) for l in ls[1:-1]) \
                or any(m.weight.shape != ((hidden, dim_in) if i == 0 else (hidden, hidden + dim_in))
                       for i, m in enumerate(mods)):
            return None
        if not ops.modsiren_gradient_supported(dim_in, hidden, len(mods), self.dim_out):
            return None
        w0_first = float(ls[0].activation.w0)
        return dict(siren_weights=[l.weight.detach() for l in ls], siren_biases=[l.bias.detach() for l in ls],
                    mod_weights=[m.weight.detach() for m in mods], mod_biases=[m.bias.detach() for m in mods],
                    w0_first=w0_first, w0=float(ls[1].activation.w0) if len(ls) > 2 else w0_first)

    def forward_with_gradient(self, x, fused: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """The generic body (autograd through THIS forward): the plain-chain kernel SirenNet dispatches to computes
        another network.  `fused` (opt-in, what Trainer(fused_modulated=True) passes): ONE kernel that carries the
        value and the tangents of a point through both stacks together (ops.modsiren_gradient) where
        `_gradient_plan` finds it serves; everything else, dim_in >= 4 included, stays the generic body."""
        if fused:
            if self.dim_out != 1:
                raise ValueError(f"forward_with_gradient needs dim_out == 1 (got {self.dim_out})")
            plan = self._gradient_plan(x)
            if plan is not None:
                with torch.no_grad():
                    return ops.modsiren_gradient(x.detach(), **plan)
        return BaseMLP.forward_with_gradient(self, x)


class HashMLP(BaseMLP):
    """Hash-grid encoder + MLP decoder (reference models.py:658-754).

    Reference decoder block: Linear -> BatchNorm1d -> activation (GELU) -> Dropout, also on
    the last layer (models.py:712-739).  Two extra keyword arguments select the tiny-MLP of
    BASELINE.json / config/hash_config.json, which is the fused MI355X hot path:
      batch_norm=False        drop BatchNorm1d (a cross-batch reduction, not shard-invariant)
      final_activation=False  linear output layer ("output_activation": "None")
    e.g. HashMLP(..., activation=nn.ReLU, batch_norm=False, final_activation=False).
    """

    def __init__(self, dim_in: int, n_levels: int, n_features_per_level: int,
                 log2_hashmap_size: int, base_resolution: Tuple[int, ...],
                 finest_resolution: Tuple[int, ...], interplation_method: str = "linear",
                 dim_hidden: int = 64, dim_out: int = 1, activation=nn.GELU,
                 dropout: float = 0.0, lr: float = 1e-4, *args, **kwargs):
        self.batch_norm = kwargs.pop("batch_norm", True)
        self.final_activation = kwargs.pop("final_activation", True)
        kwargs["_build_layers"] = False  # Q3: no dead default stack
        super().__init__(*args, **kwargs)
        self.dim_in = dim_in
        self.n_levels = n_levels
        self.n_features_per_level = n_features_per_level
        self.log2_hashmap_size = log2_hashmap_size
        self.base_resolution = base_resolution
        self.finest_resolution = finest_resolution
        self.interpolation_method = interplation_method
        self.dim_hidden = dim_hidden
        self.dim_out = dim_out
        self.activation = activation
        self.dropout = dropout
        self.lr = lr
        self.latents = []
        self.keep_latents = True

        grid_cls = (encoding.MultiResHashGrid if isinstance(base_resolution, int)
                    else encoding.MultiResHashGridV2)  # reference models.py:691-708
        self.encoder = grid_cls(dim=dim_in, n_levels=n_levels,
                                n_features_per_level=n_features_per_level,
                                log2_hashmap_size=log2_hashmap_size,
                                base_resolution=base_resolution,
                                finest_resolution=finest_resolution)
        self.encoding_dim_out = n_levels * n_features_per_level

        code = _activation_code(activation)
        self.decoder = nn.ModuleList()
        for i in range(self.n_layers):
            last = i == self.n_layers - 1
            fan_in = self.encoding_dim_out if i == 0 else dim_hidden
            fan_out = dim_out if last else dim_hidden
            act_here = self.final_activation or not last
            fuse = (not self.batch_norm) and code is not None and act_here
            mods = [FusedLinear(fan_in, fan_out, activation=code[0] if fuse else ops.ACT_IDENTITY,
                                w0=code[1] if fuse else 1.0)]
            mods.append(nn.BatchNorm1d(fan_out) if self.batch_norm else _Fused("no BatchNorm"))
            if not act_here:
                mods.append(nn.Identity())
            elif fuse:
                mods.append(_Fused(activation.__name__))
            else:
                mods.append(activation())
            mods.append(nn.Dropout(p=dropout, inplace=False))
            self.decoder.append(nn.Sequential(*mods))

    def decode(self, z):
        for block in self.decoder:
            z = block(z)
        return z

    def forward(self, x):
        return self.decode(self.encoder(x))

    def predict_step(self, batch, batch_idx):
        x, y = batch
        z = self.encoder(x)
        if self.keep_latents:
            self.latents.append(z)
        return self.decode(z)

    def get_latents(self):
        return self.latents

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        # Q3: reference checkpoints carry BaseMLP's dead default stack under `layers.*`
        for key in [k for k in state_dict if k.startswith(prefix + "layers.")]:
            state_dict.pop(key)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)


class RffNet(BaseMLP):
    """Gaussian Fourier-feature MLP (reference models.py:542-584): a frozen projection `encoder.b`, [cos | sin]
    features, then `decoder`, n_layers Linears 2 n_frequencies -> dim_hidden -> ... -> dim_out with the activation
    behind EVERY one, the last included (with ReLU the output is clamped at 0).  State-dict keys `encoder.b` and
    `decoder.{2i}.weight/bias`.  Like HashMLP (Q3) the class does not build BaseMLP's unused default `layers` stack;
    checkpoints that carry those dead `layers.*` keys still load.  Coordinates in [0, 1].
    `forward` is the encoding op and the layer ops (differentiable: training_step + autograd, and
    forward_with_gradient through the encoder's input gradient).  Inference -- `predict_step`, and `forward` under
    torch.no_grad() in eval mode -- runs ONE kernel (ops.rff_forward, csrc/rff.hip) where `_inference_plan` finds it
    serves; `fused_inference=False` keeps inference on the layer path.  `forward_with_gradient(x, fused=True)` takes
    the fused coordinate-gradient kernel (ops.rff_gradient) under the same plan."""

    def __init__(self, dim_in: int, dim_hidden: int = 128, dim_out: int = 1, n_layers: int = 8,
                 n_frequencies: int = 128, sigma: float = 10.0, activation=nn.ReLU, lr: float = 1e-4,
                 fused_inference: bool = True):
        super().__init__(dim_in=dim_in, dim_out=dim_out, dim_hidden=dim_hidden, n_layers=n_layers,
                         activation=activation, lr=lr, _build_layers=False)
        self.n_frequencies = n_frequencies
        self.sigma = sigma
        self.fused_inference = fused_inference
        self.encoder = encoding.GaussianEncoding(sigma=sigma, input_size=dim_in, encoded_size=n_frequencies)
        self.decoder = self._make_stack(2 * n_frequencies, dim_hidden, dim_out, n_layers, activation,
                                        final_activation=True)

    def forward(self, x):
        if not torch.is_grad_enabled() and not self.training:
            plan = self._inference_plan(x)
            if plan is not None:
                return ops.rff_forward(x, **plan)
        return self.decoder(self.encoder(x))

    def predict_step(self, batch, batch_idx):
        x, y = batch
        plan = self._inference_plan(x)
        if plan is not None:
            with torch.no_grad():
                return ops.rff_forward(x.detach(), **plan)
        return self(x)

    def _inference_plan(self, x):
        """Arguments of the fused inference kernel, or None where the layer path serves: a float32 (n, dim_in) tensor
        on the GPU, ReLU fused into every Linear, biases everywhere, a shape the kernel takes."""
        if not self.fused_inference or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
            return None
        linears = [m for m in self.decoder if isinstance(m, nn.Linear)]
        if len(linears) * 2 != len(self.decoder) or any(not isinstance(m, FusedLinear) for m in linears):
            return None  # (an activation without a fused epilogue runs as its own module)
        if any(m.activation_code != ops.ACT_RELU or m.bias is None for m in linears):
            return None
        b = self.encoder.b
        n_freq, dim_in = b.shape
        hidden = linears[0].weight.shape[0]
        if x.shape[1] != dim_in or linears[0].weight.shape != (hidden, 2 * n_freq) \
                or any(m.weight.shape != (hidden, hidden) for m in linears[1:-1]) \
                or linears[-1].weight.shape != (1, hidden) or len(linears) < 2:
            return None
        if not ops.rff_forward_supported(dim_in, hidden, n_freq, len(linears), self.dim_out):
            return None
        return dict(b=b.detach(), weights=[m.weight.detach() for m in linears],
                    biases=[m.bias.detach() for m in linears])

    def forward_with_gradient(self, x, fused: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """The generic body (autograd through the layer path and the encoder's input gradient).  `fused` (opt-in, what
        Trainer(fused_rff=True) passes): ONE kernel that carries the value and the tangents of a point through the
        Linears together (ops.rff_gradient) where `_inference_plan` finds the fused kernels serve -- the gradient
        kernel takes exactly the inference kernel's shapes --; everything else stays the generic body."""
        if fused:
            if self.dim_out != 1:
                raise ValueError(f"forward_with_gradient needs dim_out == 1 (got {self.dim_out})")
            plan = self._inference_plan(x)
            if plan is not None:
                with torch.no_grad():
                    return ops.rff_gradient(x.detach(), **plan)
        return BaseMLP.forward_with_gradient(self, x)

    def configure_optimizers(self):
        # torch.optim.Adam skips encoder.b (it never has a gradient); the flat buffers never take it
        self.optimizer = optim.Adam([p for p in self.parameters() if p.requires_grad], lr=self.lr)
        return self.optimizer

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        # reference checkpoints carry BaseMLP's dead default stack under `layers.*` (Q3)
        for key in [k for k in state_dict if k.startswith(prefix + "layers.")]:
            state_dict.pop(key)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)


class RealGaborLayer(nn.Module):
    """Real Gabor (WIRE) layer (reference models.py:757-788): two Linears on the same input, `freqs` and `scale`, and
    cos(w0 freqs(x)) * exp(-(c scale(x))^2).  The Linears are the MFMA kernel with the identity epilogue, the
    nonlinearity is one elementwise kernel (ops.gabor_activation); both are differentiable.  `is_first` and
    `trainable` are kept for the reference's signature and change nothing, as there."""

    def __init__(self, dim_in, dim_out, bias=True, is_first=False, w0=30.0, c=10.0, trainable=False):
        super().__init__()
        self.omega_0 = w0
        self.scale_0 = c
        self.is_first = is_first
        self.dim_in = dim_in
        self.freqs = FusedLinear(dim_in, dim_out, bias=bias)
        self.scale = FusedLinear(dim_in, dim_out, bias=bias)

    def forward(self, input):
        return ops.gabor_activation(self.freqs(input), self.scale(input), self.omega_0, self.scale_0)


class ComplexGaborLayer(nn.Module):
    """The reference's complex Gabor layer (models.py:790-834) is not built: complex weights and activations have no
    kernel here.  The name exists so that asking for it fails with a reason."""

    def __init__(self, *args, **kwargs):
        raise ValueError("ComplexGaborLayer is not supported: only real Gabor layers (RealGaborLayer) have kernels")


class GaborNet(BaseMLP):
    """Stack of Gabor layers (reference models.py:836-885): n_layers layers dim_in -> dim_hidden -> ... -> dim_out, the
    last one a Gabor layer too (the output lies in (-1, 1]), every layer with c = sigma and the same w0.  State-dict keys
    `layers.{i}.freqs.weight/bias` and `layers.{i}.scale.weight/bias`, as the reference's.
    `forward` is the layer path (differentiable: training_step + autograd, and BaseMLP.forward_with_gradient).
    Inference -- `predict_step`, and `forward` under torch.no_grad() in eval mode -- runs ONE kernel (ops.gabor_forward,
    csrc/gabor.hip) where `_inference_plan` finds it serves; `fused_inference=False` keeps inference on the layer
    path."""

    def __init__(self, layer_cls=RealGaborLayer, dim_in: int = 3, dim_hidden: int = 128, dim_out: int = 1,
                 n_layers: int = 4, sigma: float = 10.0, w0: float = 30.0, lr: float = 1e-4,
                 fused_inference: bool = True):
        if layer_cls is ComplexGaborLayer or getattr(layer_cls, "__name__", "") == "ComplexGaborLayer":
            raise ValueError("GaborNet: ComplexGaborLayer is not supported (complex weights have no kernel); use "
                             "RealGaborLayer")
        if not (isinstance(layer_cls, type) and issubclass(layer_cls, RealGaborLayer)):
            raise ValueError(f"GaborNet: layer_cls must be RealGaborLayer, got {layer_cls!r}")
        if n_layers < 1:
            raise ValueError(f"GaborNet: n_layers must be >= 1, got {n_layers}")
        super().__init__(dim_in=dim_in, dim_out=dim_out, dim_hidden=dim_hidden, n_layers=n_layers, lr=lr,
                         _build_layers=False)
        self.layer_cls = layer_cls
        self.sigma = sigma
        self.w0 = w0
        self.fused_inference = fused_inference
        self.layers = nn.Sequential(*[
            layer_cls(dim_in=dim_in if i == 0 else dim_hidden, dim_out=dim_out if i == n_layers - 1 else dim_hidden,
                      c=sigma, w0=w0) for i in range(n_layers)])

    def forward(self, x):
        if not torch.is_grad_enabled() and not self.training:
            plan = self._inference_plan(x)
            if plan is not None:
                return ops.gabor_forward(x, **plan)
        return self.layers(x)

    def predict_step(self, batch, batch_idx):
        x, y = batch
        plan = self._inference_plan(x)
        if plan is not None:
            with torch.no_grad():
                return ops.gabor_forward(x.detach(), **plan)
        return self(x)

    def _inference_plan(self, x):
        """Arguments of the fused inference kernel, or None where the layer path serves: a float32 (n, dim_in) tensor
        on the GPU, real Gabor layers with one w0 and one c, biases everywhere, a shape the kernel takes."""
        if not self.fused_inference or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
            return None
        ls = list(self.layers)
        if len(ls) < 2 or any(type(l) is not RealGaborLayer for l in ls):
            return None
        if any(not isinstance(m, FusedLinear) or m.bias is None or m.activation_code != ops.ACT_IDENTITY
               for l in ls for m in (l.freqs, l.scale)):
            return None
        if len({(float(l.omega_0), float(l.scale_0)) for l in ls}) != 1:
            return None
        hidden, dim_in = ls[0].freqs.weight.shape
        want = [(hidden, dim_in)] + [(hidden, hidden)] * (len(ls) - 2) + [(1, hidden)]
        if x.shape[1] != dim_in or any(m.weight.shape != shape for l, shape in zip(ls, want) for m in (l.freqs, l.scale)):
            return None
        if not ops.gabor_forward_supported(dim_in, hidden, len(ls), self.dim_out):
            return None
        return dict(freq_weights=[l.freqs.weight.detach() for l in ls], freq_biases=[l.freqs.bias.detach() for l in ls],
                    scale_weights=[l.scale.weight.detach() for l in ls],
                    scale_biases=[l.scale.bias.detach() for l in ls], w0=float(ls[0].omega_0), c=float(ls[0].scale_0))


def psf_table(coordinates_spacing, n_sample: int, dim_in: int):
    """(offsets (S, dim_in), weights (S,)) of PsfSirenNet (reference models.py:449-508), S = n_sample^k for
    k = len(coordinates_spacing) PSF axes: the first k input axes, the others get offset 0.  Built with the
    reference's own torch ops (linspace, ij meshgrid, Gaussian of sigma 1 / 2.3548 on +-0.5, normalised to
    sum 1): with k = dim_in = 3 the two tables are the reference's bit for bit."""
    k = len(coordinates_spacing)
    if not 1 <= k <= min(3, dim_in):
        raise ValueError(f"coordinates_spacing needs 1 to min(3, dim_in = {dim_in}) values, got {k}")
    axes = [torch.linspace(-coordinates_spacing[i], coordinates_spacing[i], n_sample) for i in range(k)]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, k)
    offsets = torch.zeros(grid.shape[0], dim_in)
    offsets[:, :k] = grid
    sigma = 1.0 / 2.3548  # could be anisotropic to reflect MRI sequences (see Kainz et al.)

    def gaussian(x, sigma):
        return torch.exp(-x * x / (2 * sigma * sigma))

    mesh = torch.meshgrid(*[torch.linspace(-0.5, 0.5, n_sample) for _ in range(k)], indexing="ij")
    psf = gaussian(mesh[0], sigma)
    for m in mesh[1:]:
        psf = psf * gaussian(m, sigma)
    psf = psf / torch.sum(psf)
    return offsets, psf.flatten()


class PsfSirenNet(SirenNet):
    """SIREN trained through the acquisition PSF (reference models.py:397-539): a target voxel is the
    network's Gaussian-weighted sum over S = n_sample^k points around it (x_to_psf_x, then psf_conv, a
    Conv1d of kernel and stride S whose weight is fixed: `psf_conv.weight`, requires_grad=False, in the
    state dict).  `forward` / `predict_step` are the plain SirenNet; only `training_step` sees the PSF.
    coordinates_spacing: the offsets' half-width per PSF axis, k = 1 .. 3 values for the first k input axes
    (the reference takes exactly 3 with dim_in = 3).  None raises (Q13).  Like the reference, the layers
    use SirenLayer's default sigma 6."""

    def __init__(self, dim_in: int = 3, dim_hidden: int = 64, dim_out: int = 1, n_layers: int = 4,
                 w0: float = 30., w0_initial: float = 30., use_bias: bool = True, final_activation=None,
                 lr: float = 1e-4, coordinates_spacing=None, n_sample: int = 5):
        if coordinates_spacing is None:
            raise ValueError("No PSF spacing defined")
        if dim_out != 1:
            raise ValueError(f"PsfSirenNet: dim_out must be 1 (psf_conv is a one-channel Conv1d), got {dim_out}")
        if int(n_sample) < 1:
            raise ValueError(f"n_sample must be >= 1, got {n_sample}")
        offsets, psf = psf_table(coordinates_spacing, int(n_sample), dim_in)
        super().__init__(dim_in=dim_in, dim_hidden=dim_hidden, dim_out=dim_out, n_layers=n_layers, w0=w0,
                         w0_initial=w0_initial, use_bias=use_bias, final_activation=final_activation, lr=lr)
        self.n_sample = int(n_sample)
        self.coordinates_spacing = coordinates_spacing
        self.psf_coordinates = offsets  # a plain attribute, as in the reference (not in the state dict)
        self._psf_device = {}
        psf_conv = nn.Conv1d(in_channels=1, out_channels=1, kernel_size=len(psf), stride=len(psf), padding=0,
                             bias=False)  # holds the weight; its math runs in ops.psf_conv
        psf_conv.weight = nn.Parameter(psf.unsqueeze(0).unsqueeze(0), requires_grad=False)
        self.psf_conv = psf_conv

    @property
    def n_psf(self) -> int:
        return self.psf_coordinates.shape[0]

    def psf_offsets(self, device) -> torch.Tensor:
        """psf_coordinates on `device` (uploaded once)."""
        key = str(device)
        t = self._psf_device.get(key)
        if t is None:
            t = self.psf_coordinates.to(device).contiguous()
            self._psf_device[key] = t
        return t

    def psf_weights(self) -> torch.Tensor:
        return self.psf_conv.weight.detach().reshape(-1)

    def forward(self, x, mods=None):
        return super().forward(x)

    def x_to_psf_x(self, x: torch.Tensor):
        """Row b S + k = x[b] + psf_coordinates[k] (reference models.py:520-526), one kernel."""
        return ops.psf_expand_ad(x, self.psf_offsets(x.device))

    def training_step(self, batch, batch_idx):
        x, y = batch
        z = self(self.x_to_psf_x(x))
        z = ops.psf_conv(z, self.psf_conv.weight)
        loss = self.criterion(y, z)
        self.log("train_loss", loss)
        return loss

    def configure_optimizers(self):
        # torch.optim.Adam skips psf_conv.weight (it never has a gradient); the flat buffers never take it
        self.optimizer = optim.Adam([p for p in self.parameters() if p.requires_grad], lr=self.lr)
        return self.optimizer
