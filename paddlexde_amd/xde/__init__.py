from .base_ode import BaseODE  # noqa: F401
from .base_xde import BaseXDE  # noqa: F401
from .base_dde import BaseDDE, HistoryIndex  # noqa: F401,E402
from .base_sde import BaseSDE, SDELinearHead  # noqa: F401,E402
from .base_cde import BaseCDE, CDEField, CDELinearHead, CdeControlContractFn  # noqa: F401,E402
from .mlp_field import MLPField  # noqa: F401,E402
