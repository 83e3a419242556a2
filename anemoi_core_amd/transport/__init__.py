"""The transport (diffusion) family's settings, schedules, sources and objectives - mirror of the reference's ``anemoi.models.transport``
for the EDM diffusion objective."""
from .objectives import EDMDiffusionModelObjective, TransportModelObjective, get_transport_model_objective  # noqa: F401
from .schedules import (SIGMA_SCHEDULES, CosineSigmaSchedule, ExponentialSigmaSchedule, KarrasSigmaSchedule,  # noqa: F401
                        LinearSigmaSchedule)
from .settings import EdmSettings, NoiseConditioningSettings, TransportSourceSettings  # noqa: F401
from .sources import TransportSourceBuilder, TransportSourceSpec, sampling_source_specs  # noqa: F401
