from .transport_samplers import DIFFUSION_SAMPLERS, DPMpp2MSampler, EDMDiffusionSampler, EDMHeunSampler  # noqa: F401
