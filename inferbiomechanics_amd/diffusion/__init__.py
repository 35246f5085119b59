from .sampler import ConditionalDDIMSampler, DDIMSampler, StitchedDDIMSampler, StochasticStitchedSampler  # noqa: F401
from .schedule import stitch_layout  # noqa: F401
