"""Fixed-grid solver classes (the names the reference exports from this package)."""
from . import adams, euler, grheun, heun, midpoint, milstein, rheun, rk4, srk

RK4, Euler, Midpoint = rk4.RK4, euler.Euler, midpoint.Midpoint
AdamsBashforthMoulton = adams.AdamsBashforthMoulton
Milstein = milstein.Milstein
SRK = srk.SRK
ReversibleHeun = rheun.ReversibleHeun
Heun = heun.Heun
GeneralReversibleHeun = grheun.GeneralReversibleHeun

__all__ = ["AdamsBashforthMoulton", "Euler", "GeneralReversibleHeun", "Heun", "Midpoint", "Milstein", "RK4", "ReversibleHeun", "SRK"]
