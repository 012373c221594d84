"""Decoder likelihood selection mirroring pyroved/utils/prob.py:5-37, plus 'poisson_log' for count data and 'categorical' for
label maps."""
import torch
import torch.distributions as td


class _Sampler:
    """Callable like the reference's lambdas (x -> distribution object); `.name` /
    `.decoder_sig` tell the HIP path which likelihood kernel (enum pv_lik) to run."""
    def __init__(self, name, decoder_sig):
        self.name = name
        self.decoder_sig = float(decoder_sig)

    def __call__(self, x):
        if self.name == "bernoulli":
            return td.Bernoulli(x, validate_args=False)
        if self.name == "continuous_bernoulli":
            return td.ContinuousBernoulli(x)
        if self.name == "poisson_log":             # x is the log-rate (no output sigmoid); clamped like enum pv_lik's comment says
            return td.Poisson(torch.exp(x.clamp(max=30)), validate_args=False)
        return td.Normal(x, self.decoder_sig)


class _ChannelCategorical:
    """The categorical likelihood over the trailing C values of every position of a flattened channel-last row of logits
    (..., positions * C).  log_prob(x) returns the PER-VALUE terms x_c (a_c - logsumexp_c a) in x's shape, so that .sum(-1) (or
    to_event(1)) gives the row's log-likelihood like the per-value likelihoods' log_prob does; `probs` are the class
    probabilities in the same layout.  No multinomial coefficient: it is 0 for one-hot x and depends on the data only otherwise."""
    def __init__(self, logits, channels):
        if logits.shape[-1] % channels != 0:
            raise ValueError("the last dimension (%d) must be a multiple of channels=%d" % (logits.shape[-1], channels))
        self.logits, self.channels = logits, channels
        grouped = logits.reshape(*logits.shape[:-1], -1, channels)
        self._logp = (grouped - torch.logsumexp(grouped, -1, keepdim=True)).reshape(logits.shape)

    @property
    def probs(self):
        return self._logp.exp()

    def log_prob(self, x):
        return x * self._logp


class _CategoricalSampler(_Sampler):
    """'categorical': the C channel values of a position are the logits of one categorical observation (one-hot or soft labels)."""
    def __init__(self, channels):
        super().__init__("categorical", 0.5)
        self.channels = int(channels)

    def __call__(self, x):
        return _ChannelCategorical(x, self.channels)


def only_ivae_sampler(sampler: str, model_name: str) -> None:
    """The models that score every value on its own refuse the joint likelihood by name, before anything is built."""
    if sampler == "categorical":
        raise ValueError("sampler_d='categorical' is implemented for models.iVAE(..., channels=C) only (not for %s)" % model_name)


def get_sampler(sampler: str, **kwargs: float):
    """'bernoulli', 'continuous_bernoulli', 'gaussian' (decoder_sig kwarg, default 0.5), 'poisson_log': a Poisson
    parameterised by its log-rate (the decoder's output, sigmoid_d=False), the observation model for counts — or 'categorical'
    (channels kwarg, C >= 2): the C values of a position are the logits of ONE categorical observation (sigmoid_d=False), the
    observation model for label maps; its object's log_prob(x) returns the per-value terms x_c (a_c - logsumexp_c a) over the
    flattened channel-last row."""
    names = ["bernoulli", "continuous_bernoulli", "gaussian", "poisson_log", "categorical"]
    if sampler not in names:
        raise KeyError("Select between the following decoder samplers: {}".format(names))
    if sampler == "categorical":
        channels = kwargs.get("channels", None)
        if isinstance(channels, bool) or not isinstance(channels, int) or channels < 2:
            raise ValueError("sampler 'categorical' needs channels >= 2, the number of classes per position (got channels=%r)"
                             % (channels,))
        return _CategoricalSampler(channels)
    return _Sampler(sampler, kwargs.get("decoder_sig", 0.5))
