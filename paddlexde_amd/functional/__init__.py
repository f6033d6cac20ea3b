from .ddeint import ddeint  # noqa: F401
from .ddeint_adjoint import ddeint_adjoint  # noqa: F401
from .odeint import odeint  # noqa: F401
from .odeint_adjoint import AdjointProblem, odeint_adjoint  # noqa: F401
from .sdeint import sdeint  # noqa: F401
from .sdeint_adjoint import sdeint_adjoint  # noqa: F401
from .cdeint import cdeint, cdeint_adjoint  # noqa: F401
from .ddeint_steps import ddeint_steps  # noqa: F401
