"""
ivae.py — variational autoencoder that enforces invariance to rotation, translation
and scale; host-side mirror of pyroved/models/ivae.py:27-310.

Same constructor signature, attributes (encoder_z, decoder, sampler_d, z_dim, c_dim,
grid, t_prior, sc_prior, coord, ndim, invariances, device), parameter initialisation
order (so `seed` reproduces the reference's initial weights bit-for-bit) and
inference API (encode / decode / manifold2d / split_latent).

`model()` / `guide()` are Pyro programs in the reference; here the SVI objective they
define is evaluated by the HIP library (trainers.SVItrainer -> engine.loss_and_grads ->
pv_ivae_loss_and_grads), so they are kept only as thin hooks that run the same
computation and return the ELBO terms.
"""
from typing import Optional, Tuple, Union, List

import torch

from .base import baseVAE
from ..nets import fcDecoderNet, fcEncoderNet, sDecoderNet
from ..utils import get_sampler, set_deterministic_mode


def _plot_manifold(ndim, loc, d, grid_x, grid_y, kwargs):
    """The plot=True tail shared by every manifold2d (models/ivae.py:302-309)."""
    from ..utils.viz import plot_img_grid, plot_spect_grid
    dd = d[0] if isinstance(d, (list, tuple)) else d
    if ndim == 2:
        plot_img_grid(loc, dd, extent=[grid_x.min(), grid_x.max(), grid_y.min(), grid_y.max()], **kwargs)
    elif ndim == 1:
        plot_spect_grid(loc, dd, **kwargs)


class iVAE(baseVAE):
    """
    Variational autoencoder that enforces rotational, translational,
    and scale invariances.

    Args:
        data_dim: (height, width) or (length,)
        latent_dim: number of latent dimensions (content)
        invariances: e.g. ['r'], ['r', 't'], ['r', 't', 's'], ['t'] (1D), None (vanilla VAE)
        c_dim: "feature dimension" of the class vector for class-conditioned VAEs
        hidden_dim_e / hidden_dim_d: hidden layer widths of encoder / decoder (default [128, 128])
        activation: 'tanh' (default), 'lrelu', 'softplus', 'relu', 'gelu'
        sampler_d: 'bernoulli' (default), 'continuous_bernoulli', 'gaussian', or 'poisson_log' for count data: a Poisson
            whose log-rate is the decoder's output (needs sigmoid_d=False; decode / manifold2d return the rate), or
            'categorical' for label maps (channels=C >= 2, sigmoid_d=False): the C values of a position are ONE observation
            on the simplex — one-hot labels (utils.onehot_channels) or soft ones — and the decoder's C outputs its logits:
            log p(x | z) = sum over positions of sum_c x_c log softmax(a)_c (no multinomial coefficient: 0 for one-hot x,
            data-only otherwise); decode / manifold2d return the class probabilities.  Observation weights multiply each
            term x_c log p_c.  iVAE with its own fully connected networks only
        sigmoid_d: sigmoid at the decoder output (default True)
        seed: seed used in torch.manual_seed(seed)
        channels: values per grid position, 1 .. 8 (default 1).  With C > 1 the data is channel-last, x of shape
            (B, *data_dim, C): data_dim stays the grid's shape, so 1-D spectra take channels too, (B, l, C).  The spatial
            decoder's output layer becomes Linear(hidden, C) (decoder.out.weight (C, hidden), decoder.out.bias (C,)), the
            likelihood and sigmoid_d apply per value, log p(x | z) sums over positions and channels, and rotation, shift and
            scale are shared by the channels; decode / manifold2d return (n, *data_dim, C).  The encoder sees the flattened
            (B, prod(data_dim) * C [+ c_dim]).  Trains on the layer-by-layer HIP kernels at fp32 (SVItrainer(precision="bf16")
            is refused); set_encoder with a convolutional or user-defined module, set_decoder and the Pyro-program hooks
            model() / guide() are refused.  channels=1 is the single-channel model in every respect.

    Keyword Args:
        device, dx_prior, dy_prior, sc_prior, decoder_sig — as in the reference.
    """

    _multichannel = True

    def __init__(
        self,
        data_dim: Tuple[int],
        latent_dim: int = 2,
        invariances: List[str] = None,
        c_dim: int = 0,
        hidden_dim_e: List[int] = None,
        hidden_dim_d: List[int] = None,
        activation: str = "tanh",
        sampler_d: str = "bernoulli",
        sigmoid_d: bool = True,
        seed: int = 1,
        channels: int = 1,
        **kwargs: Union[str, float]
         ) -> None:
        args = (data_dim, invariances)
        super(iVAE, self).__init__(*args, channels=channels, **kwargs)
        if sampler_d == "categorical":
            # one observation per position: its C values are class logits, so there must be classes and no output sigmoid
            if self.channels < 2:
                raise ValueError("sampler_d='categorical' needs channels >= 2, the number of classes per position "
                                 "(got channels=%d)" % self.channels)
            if sigmoid_d:
                raise ValueError("sampler_d='categorical' needs sigmoid_d=False (the decoder's outputs are the class logits)")

        # same RNG consumption as the reference (models/ivae.py:140-154): seed, then the
        # encoder's Linear layers, then the decoder's, all on the CPU generator
        set_deterministic_mode(seed)

        # channels > 1: the fully connected nets see (*data_dim, C), channel-last; the spatial decoder keeps the grid's shape
        # and emits C values per position.  channels == 1 builds exactly what it always did
        C = self.channels
        full_dim = data_dim if C == 1 else (*data_dim, C)
        self.encoder_z = fcEncoderNet(
            full_dim, latent_dim + self.coord, c_dim, hidden_dim_e,
            activation, softplus_out=True
        )
        if 0 < self.coord < 5:
            self.decoder = sDecoderNet(
                data_dim, latent_dim, c_dim, hidden_dim_d,
                activation, sigmoid_out=sigmoid_d, **({} if C == 1 else {"channels": C})
            )
        else:
            self.decoder = fcDecoderNet(
                full_dim, latent_dim, c_dim, hidden_dim_d,
                activation, sigmoid_out=sigmoid_d
            )
        self.sampler_d = get_sampler(sampler_d, **{**kwargs, "channels": C})

        self.z_dim = latent_dim + self.coord
        self.c_dim = c_dim

        self.to(self.device)

    # ---------------------------------------------------------------- ELBO hooks
    def elbo_terms(self, x: torch.Tensor, y: Optional[torch.Tensor] = None,
                   eps: Optional[torch.Tensor] = None, **kwargs: float):
        """Evaluates guide + model once (no gradients, no update) through the HIP library and
        returns dict(loss, ll, logpz, logqz) as python floats.  `eps` (B, z_dim) is the
        standard-normal draw of the guide; drawn on the CPU generator when omitted.
        Replaces tracing `model`/`guide` with Pyro (models/ivae.py:165-221).
        image_weights=w (an engine made with image_weights=True): the batch's per-image observation weights."""
        eng = self.engine()
        x = x.to(eng.device, torch.float32)
        if eps is None:
            eps = torch.empty(x.shape[0], self.z_dim).normal_()
        extra = {"image_weights": kwargs["image_weights"]} if kwargs.get("image_weights", None) is not None else {}
        eng.loss_and_grads(x, eps.to(eng.device, torch.float32), kwargs.get("scale_factor", 1.),
                           None if y is None else y.to(eng.device, torch.float32), want_grads=False, **extra)
        s = eng.scalars.cpu().tolist()
        return dict(loss=s[0], ll=s[1], logpz=s[2], logqz=s[3])

    # ---------------------------------------------------------------- held-out log-evidence
    LOG_EVIDENCE_ROW_CAP = 1 << 19     # decoder rows (P * batch * positions) of one chunk: see log_evidence

    @classmethod
    def _evidence_chunk(cls, num_samples: int, batch: int, positions: int) -> int:
        """The default `chunk` of log_evidence: the largest P <= min(num_samples, 1024) with P * batch * positions <=
        LOG_EVIDENCE_ROW_CAP, at least 1."""
        return max(1, min(int(num_samples), 1024, cls.LOG_EVIDENCE_ROW_CAP // max(1, int(batch) * int(positions))))

    def _evidence_positions(self) -> int:
        """Decoder rows per sample: the grid positions of the spatial decoder, 1 for the vanilla decoder (one row per sample)."""
        import math
        return math.prod(int(d) for d in self.data_dim) if 0 < self.coord < 5 else 1

    def _evidence_schedule(self, n: int, num_samples: int, chunk: Optional[int], batch_size: int, eps: Optional[torch.Tensor]):
        """The work list of log_evidence as (lo, hi, first, eps_chunk): image batches [lo, hi) in order (outer), for each the chunks of
        particles in order (inner), eps_chunk (P, hi - lo, z_dim) on the CPU — the caller's slice, or drawn here in exactly that
        order with torch.empty(P, hi - lo, z_dim).normal_() on the CPU generator."""
        for lo in range(0, n, batch_size):
            hi = min(n, lo + batch_size)
            P = int(chunk) if chunk is not None else self._evidence_chunk(num_samples, hi - lo, self._evidence_positions())
            for k0 in range(0, num_samples, P):
                k1 = min(num_samples, k0 + P)
                e = eps[k0:k1, lo:hi] if eps is not None else torch.empty(k1 - k0, hi - lo, self.z_dim).normal_()
                yield lo, hi, k0 == 0, e

    def log_evidence(self, x: torch.Tensor, y: Optional[torch.Tensor] = None, num_samples: int = 64, chunk: Optional[int] = None,
                     eps: Optional[torch.Tensor] = None, return_ess: bool = False, batch_size: Optional[int] = None):
        """Held-out log-evidence per image: the K-sample importance-weighted estimate ("IWAE-K", K = num_samples, beta = 1)
            log p^(x_b) = logsumexp_k [log p(x_b | z_kb [, y_b]) + log N(z_kb; 0, 1) - log N(z_kb; mu_b, sigma_b)] - log K,
        z_kb = mu_b + sigma_b eps_kb, with every normaliser of the likelihood (the Poisson's -sum lgamma(x + 1) per image included).
        Returns a CPU float32 tensor (n,); with return_ess=True also the effective sample size (n,), (sum w)^2 / sum w^2 in [1, K].
        Runs through the HIP library (pv_ivae_evidence_accumulate): the encoder once per image batch, forward-only decoder launches.

        batch_size: images per call, as in encode (default 100).  chunk: particles per call; the estimate streams over
        ceil(num_samples / chunk) calls against a running (max, sum, sum of squares) per image, the last chunk may be smaller.
        Default: the largest P <= min(num_samples, 1024) with P * batch * positions <= 2^19 = 524 288 decoder rows (positions: grid
        points of the spatial decoder, 1 for the vanilla one), which keeps the evidence workspace in the hundreds of MB on every
        path: about 1.5 kB per row on the layer-by-layer kernels with 128-wide layers (0.8 GB at the cap), about 50 B per row on
        the fused decoder kernels — there a larger explicit chunk (16 at 28x28, batch 256: 160 MB) is faster, DESIGN.md 4.20.
        eps: optional (num_samples, n, z_dim) standard-normal draws.  When omitted they are drawn on the CPU generator with
        torch.empty(P, b, z_dim).normal_() — one draw per call, image batches outer and chunks inner — so a seed fixes the estimate.
        Precision: the engine's — fused=2 and fused=0 are fp32-class, fused=3 (SVItrainer(precision="bf16")) evaluates with the bf16
        forward; an engine with fused=1 or fused_channels=True evaluates on the layer-by-layer plan (fused=0): both are fp32.
        Not for engines configured with pixel_weights / image_weights (no kernel applies observation weights to several particles)."""
        num_samples = int(num_samples)
        if num_samples < 1:
            raise ValueError("log_evidence: num_samples must be >= 1 (got %d)" % num_samples)
        if chunk is not None and not 1 <= int(chunk) <= 1024:
            raise ValueError("log_evidence: chunk must be in 1 .. 1024 particles (got %r)" % (chunk,))
        if self.c_dim > 0 and y is None:
            raise ValueError("log_evidence: class-conditioned model (c_dim=%d) needs y" % self.c_dim)
        n = int(x.shape[0])
        if eps is not None and tuple(eps.shape) != (num_samples, n, self.z_dim):
            raise ValueError("log_evidence: eps must have shape (num_samples, n, z_dim) = (%d, %d, %d) (got %s)"
                             % (num_samples, n, self.z_dim, tuple(eps.shape)))
        eng = self.engine()
        eng._check_evidence()
        batch_size = 100 if batch_size is None else int(batch_size)
        out, ess, state, cur = [], [], None, None

        def flush():
            lp, es = eng.log_evidence_finish(state, num_samples, return_ess)
            out.append(lp)
            if return_ess:
                ess.append(es)

        for lo, hi, first, e in self._evidence_schedule(n, num_samples, chunk, batch_size, eps):
            if first:
                if state is not None:
                    flush()
                cur = (x[lo:hi].to(eng.device, torch.float32), None if y is None else y[lo:hi].to(eng.device, torch.float32))
                state = None
            state = eng.log_evidence_chunk(cur[0], e.to(eng.device, torch.float32), cur[1], state, first)
        if state is not None:
            flush()
        res = torch.cat(out).cpu() if out else torch.empty(0)
        return (res, torch.cat(ess).cpu()) if return_ess else res

    def model(self, x: torch.Tensor, y: Optional[torch.Tensor] = None, **kwargs: float) -> None:
        """p(x|z)p(z) as a Pyro program (models/ivae.py:165-202) — for users with pyro-ppl (poutine.trace, custom ELBOs,
        pyro.infer.SVI); raises NotImplementedError without it.  SVItrainer evaluates the same objective in HIP kernels
        and does not go through here (iVAE.elbo_terms does neither)."""
        from ._pyro_programs import ivae_model
        self._no_pyro_channels("model")
        return ivae_model(self, x, y, **kwargs)

    def guide(self, x: torch.Tensor, y: Optional[torch.Tensor] = None, **kwargs: float) -> None:
        """q(z|x) as a Pyro program (models/ivae.py:204-221); see `model`."""
        from ._pyro_programs import ivae_guide
        self._no_pyro_channels("guide")
        return ivae_guide(self, x, y, **kwargs)

    def _no_pyro_channels(self, what: str) -> None:
        if self.channels != 1:
            raise ValueError("channels=%d: the Pyro-program hook %s() is written for single-channel data; train with "
                             "SVItrainer (the HIP path)" % (self.channels, what))

    def split_latent(self, z: torch.Tensor) -> Tuple[torch.Tensor]:
        """Split latent variable into parts associated with coordinate transformations
        (rotation and/or translation and/or scale) and image content."""
        return self._split_latent(z)

    # ---------------------------------------------------------------- inference
    def encode(self, x_new: torch.Tensor, y: torch.Tensor = None, **kwargs: int) -> torch.Tensor:
        """Encodes data with the trained encoder: returns (z_loc, z_scale) on the CPU.  The last
        latent_dim columns are the content latents; the first ones are rotation, dx, dy, scale
        (models/ivae.py:230-256).  kwargs: batch_size."""
        enc_args = [x_new, y] if y is not None else [x_new, ]
        z = self._encode(*enc_args, **kwargs)
        z_loc, z_scale = z.split(self.z_dim, 1)
        return z_loc, z_scale

    def decode(self, z: torch.Tensor, y: torch.Tensor = None, **kwargs: int) -> torch.Tensor:
        """Decodes a batch of (content) latent coordinates into the data space
        (models/ivae.py:258-275).  kwargs: batch_size, angle, shift, scale."""
        z = z.to(torch.float32)
        if y is not None:
            z = torch.cat([z.cpu(), y.to(torch.float32).cpu()], -1)
        return self._decode(z.cpu(), **kwargs)

    def manifold2d(self, d: int, y: torch.Tensor = None, plot: bool = True,
                   **kwargs: Union[str, int, float]) -> torch.Tensor:
        """Decodes a d x d grid of the 2-D latent space (models/ivae.py:277-310).  The grid is the
        reference's generate_latent_grid: inverse normal CDF of linspace(0.05, 0.95, d) unless
        z_coord=[z1, z2, z3, z4] is given; plot=True draws the mosaic (utils.plot_img_grid / plot_spect_grid; of a
        multi-channel model: channel `channel`, default 0)."""
        import torch.distributions as td
        if isinstance(d, int):
            d = [d, d]
        z_coord = kwargs.get("z_coord")
        if z_coord:
            z1, z2, z3, z4 = z_coord
            grid_x = torch.linspace(z2, z1, d[0])
            grid_y = torch.linspace(z3, z4, d[1])
        else:
            grid_x = td.Normal(0, 1).icdf(torch.linspace(0.95, 0.05, d[0]))
            grid_y = td.Normal(0, 1).icdf(torch.linspace(0.05, 0.95, d[1]))
        z = []
        for xi in grid_x:
            for yi in grid_y:
                z.append(torch.tensor([xi, yi]).float().unsqueeze(0))
        z = torch.cat(z)
        if self.c_dim > 0:
            if y is None:
                raise ValueError("To generate a manifold pass a conditional vector y")
            y = y.unsqueeze(1) if 0 < y.ndim < 2 else y
            loc = self.decode(z, y.expand(z.shape[0], *y.shape[1:]), **kwargs)
        else:
            loc = self.decode(z, **kwargs)
        if plot:
            # (multi-channel: the mosaic shows one channel, channel=0 unless given)
            shown = loc if self.channels == 1 else loc[..., int(kwargs.get("channel", 0))]
            _plot_manifold(self.ndim, shown, d, grid_x, grid_y, {k: v for k, v in kwargs.items() if k != "channel"})
        return loc

    def predict_on_latent(self, train_data, gp_labels, gp_iterations: int = 1, d: int = 12, plot: bool = False):
        """Gaussian-process regression of labels over the latent space, evaluated on the d x d latent grid
        (models/ivae.py:312-364): encode, fit utils.gp_model on the encoded means, predict on
        utils.generate_latent_grid(d), decode the grid.  Returns ((z, z_decoded), predictions)."""
        from ..utils import generate_latent_grid
        from ..utils.gp import gp_model
        X = torch.as_tensor(train_data, dtype=torch.float32)
        y = torch.as_tensor(gp_labels, dtype=torch.float32)
        encoded_X = self.encode(X)[0]
        gpr = gp_model(input_dim=encoded_X.shape[1], encoded_X=encoded_X, y=y, gp_iterations=gp_iterations)
        z, _ = generate_latent_grid(d)
        z = torch.as_tensor(z, dtype=torch.float32)
        gpr.eval()
        with torch.no_grad():
            predictions, _ = gpr(z)
        z_decoded = self.manifold2d(d, plot=False)
        if plot:
            import matplotlib.pyplot as plt
            self.manifold2d(d=d, cmap='viridis')
            plt.figure(figsize=(8, 8))
            heatmap = plt.imshow(predictions.reshape(d, d), cmap='viridis', aspect='auto')
            plt.colorbar(heatmap, label='Prediction Value')
            plt.xticks(fontsize=14)
            plt.yticks(fontsize=14)
            plt.xlabel("$z_1$", fontsize=14)
            plt.ylabel("$z_2$", fontsize=14)
            plt.title('Predictions Visualization')
            plt.show()
        return (z, z_decoded), predictions
