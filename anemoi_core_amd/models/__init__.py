from .encoder_processor_decoder import AnemoiModelEncProcDec  # noqa: F401
from .ens_encoder_processor_decoder import AnemoiEnsModelEncProcDec  # noqa: F401
from .transport_encoder_processor_decoder import AnemoiTransportModelEncProcDec  # noqa: F401
