from .cem_sampler import CEMSampler
from .gaussian_sampler import GaussianCEMSampler
from .autograsp_sampler import AutograspSampler
from .correlated_noise import CorrelatedNoiseSampler
from .philox_gaussian_sampler import PhiloxGaussianCEMSampler
