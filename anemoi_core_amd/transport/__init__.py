"""The transport (diffusion) family's settings, schedules, sources and objectives - mirror of the reference's ``anemoi.models.transport``
for the EDM diffusion objective."""
from .objectives import EDMDiffusionModelObjective, TransportModelObjective, get_transport_model_objective  # noqa: F401
from .paths import edm_loss_weight, karras_sigma_from_unit_time  # noqa: F401
from .schedules import (SIGMA_SCHEDULES, SIGMA_TRAINING_DISTRIBUTIONS, CosineSigmaSchedule, CosineSigmaTrainingDistribution,  # noqa: F401
                        ExponentialSigmaSchedule, ExponentialSigmaTrainingDistribution, KarrasSigmaSchedule, KarrasSigmaTrainingDistribution,
                        LinearSigmaSchedule, LinearSigmaTrainingDistribution, SigmaTrainingDistribution, cosine_sigma_from_unit_time,
                        exponential_sigma_from_unit_time)
from .settings import EdmSettings, NoiseConditioningSettings, TransportSourceSettings  # noqa: F401
from .sources import TransportSourceBuilder, TransportSourceSpec, sampling_source_specs  # noqa: F401
