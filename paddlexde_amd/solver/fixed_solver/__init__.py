"""Fixed-grid solver classes (the names the reference exports from this package)."""
from . import adams, euler, midpoint, milstein, rheun, rk4, srk

RK4, Euler, Midpoint = rk4.RK4, euler.Euler, midpoint.Midpoint
AdamsBashforthMoulton = adams.AdamsBashforthMoulton
Milstein = milstein.Milstein
SRK = srk.SRK
ReversibleHeun = rheun.ReversibleHeun

__all__ = ["AdamsBashforthMoulton", "Euler", "Midpoint", "Milstein", "RK4", "ReversibleHeun", "SRK"]
