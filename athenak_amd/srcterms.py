"""SourceTerms -- physical source terms of a fluid, <hydro_srcterms> / <mhd_srcterms>
(src/srcterms/srcterms.hpp, srcterms.cpp, srcterms_newdt.cpp).

On this path: const_accel (constant acceleration) and ism_cooling (optically thin ISM cooling and heating, ideal gas,
needs <units>).  Both are applied by one kernel launch per stage (akmi_srcterms_apply, csrc/akmi_srcterms.hip) from
the task `srctrms` between the RK update and the send of the conserved variables; the cooling time step comes from
akmi_srcterms_newdt.  self_gravity (akmi_mg_selfgravity, csrc/akmi_mg.hip) comes after them and needs the <gravity>
block (gravity.py); rel_cooling and rad_beam stop with a message, and so does self_gravity without <gravity>.
"""
import torch

from . import capi
from .mesh import FLT_MAX

REFUSED = ("rel_cooling", "self_gravity", "rad_beam")


def srcterms_deck_checks(pin):
    """what a source-term block may not ask for; called by both hosts before anything is allocated"""
    for fluid in ("hydro", "mhd"):
        blk = fluid + "_srcterms"
        if not (pin.DoesBlockExist(fluid) and pin.DoesBlockExist(blk)):
            continue
        for key in REFUSED:
            if key == "self_gravity" and pin.DoesBlockExist("gravity"):
                continue             # (the reference exits on the null pgrav without the block; with it the term is built)
            if pin.DoesParameterExist(blk, key) and pin.GetBoolean(blk, key):
                raise RuntimeError("### FATAL ERROR <%s>/%s = true is not on this path (const_accel and ism_cooling "
                                   "are)" % (blk, key))
        if pin.DoesParameterExist(blk, "const_accel") and pin.GetBoolean(blk, "const_accel"):
            pin.GetReal(blk, "const_accel_val")
            d = pin.GetInteger(blk, "const_accel_dir")
            if d < 1 or d > 3:
                raise RuntimeError("### FATAL ERROR <%s>/const_accel_dir must be 1, 2 or 3" % blk)
        if pin.DoesParameterExist(blk, "ism_cooling") and pin.GetBoolean(blk, "ism_cooling"):
            pin.GetReal(blk, "hrate")
            if pin.GetString(fluid, "eos") != "ideal":
                raise RuntimeError("### FATAL ERROR <%s>/ism_cooling = true needs the ideal-gas EOS (<%s>/eos = %s)"
                                   % (blk, fluid, pin.GetString(fluid, "eos")))
            if not pin.DoesBlockExist("units"):
                # (the reference dereferences the null punit here)
                raise RuntimeError("### FATAL ERROR <%s>/ism_cooling = true needs a <units> block (length_cgs, "
                                   "mass_cgs, time_cgs, mu)" % blk)
            if pin.DoesParameterExist("coord", "general_rel") and pin.GetBoolean("coord", "general_rel"):
                raise RuntimeError("### FATAL ERROR <units> from a black-hole mass (<coord>/general_rel = true) is "
                                   "not on this path")


def cooling_units(punit):
    """(temp_unit, cooling_unit, heating_unit) of srcterms.cpp:149-154"""
    temp_unit = punit.temperature_cgs()
    n_unit = punit.density_cgs()/punit.mu()/punit.atomic_mass_unit_cgs
    cooling_unit = punit.pressure_cgs()/punit.time_cgs()/n_unit/n_unit
    heating_unit = punit.pressure_cgs()/punit.time_cgs()/n_unit
    return temp_unit, cooling_unit, heating_unit


class SourceTerms:
    """srcterms.cpp:37-80: keys and defaults of the block"""

    def __init__(self, block, fluid, pin):
        self.pmy_fluid = fluid
        self.block = block
        self.const_accel = pin.GetOrAddBoolean(block, "const_accel", False)
        self.ism_cooling = pin.GetOrAddBoolean(block, "ism_cooling", False)
        self.rel_cooling = pin.GetOrAddBoolean(block, "rel_cooling", False)
        self.rad_beam = pin.GetOrAddBoolean(block, "rad_beam", False)
        self.self_gravity = pin.GetOrAddBoolean(block, "self_gravity", False)
        self.dtnew = FLT_MAX
        self.const_accel_val, self.const_accel_dir, self.hrate = 0.0, 1, 0.0
        if self.const_accel:
            self.const_accel_val = pin.GetReal(block, "const_accel_val")
            self.const_accel_dir = pin.GetInteger(block, "const_accel_dir")
        if self.ism_cooling:
            self.hrate = pin.GetReal(block, "hrate")
        eos = fluid.peos.eos_data
        tu = cu = hu = 1.0
        if self.ism_cooling:
            tu, cu, hu = cooling_units(fluid.pmy_pack.punit)
        self.temp_unit, self.cooling_unit, self.heating_unit = tu, cu, hu
        self.c = capi.SrcTerms(1 if self.const_accel else 0, self.const_accel_dir, 1 if self.ism_cooling else 0, 0,
                               self.const_accel_val, self.hrate, eos.gamma, tu, cu, hu)
        self.dt_dev = None

    @property
    def active(self):
        return self.const_accel or self.ism_cooling or self.self_gravity

    def ApplySrcTerms(self, w0, bdt_beta, dt, u0):
        """srcterms.cpp:93-101: bdt = beta*dt, formed in the kernel; SelfGravity last"""
        f = self.pmy_fluid
        if self.const_accel or self.ism_cooling:
            capi.check(f.L.akmi_srcterms_apply(f.pack_c, self.c, bdt_beta, dt, None, w0, u0, capi._stream()),
                       "srcterms_apply")
        if self.self_gravity:
            self.SelfGravity(w0, bdt_beta*dt, u0)

    def SelfGravity(self, w0, bdt, u0):
        """srcterms.cpp:215-310: phi of the last Solve, the Godunov mass fluxes of this stage (ideal gas)"""
        f = self.pmy_fluid
        pgrav = getattr(f.pmy_pack, "pgrav", None)
        if pgrav is None:
            raise RuntimeError("### ERROR in SourceTerms::SelfGravity\nself_gravity source term enabled but pgrav is null")
        fl = f.uflx
        if fl is None:
            raise RuntimeError("### FATAL ERROR self_gravity needs the flux arrays of the task-granular path")
        face = 1 if fl.x1f.shape[-1] == u0.shape[-1] + 1 else 0
        capi.check(f.L.akmi_mg_selfgravity(f.pack_c, face, bdt, w0, pgrav.phi, fl.x1f, fl.x2f, fl.x3f, u0,
                                           capi._stream()), "mg_selfgravity")

    def NewTimeStep(self, w0):
        """srcterms_newdt.cpp:25-72"""
        f = self.pmy_fluid
        if not self.ism_cooling:
            self.dtnew = FLT_MAX
            return
        if self.dt_dev is None:
            self.dt_dev = torch.zeros(1, dtype=torch.float64, device=f.device)
        capi.check(f.L.akmi_srcterms_newdt(f.pack_c, self.c, w0, self.dt_dev, capi._stream()), "srcterms_newdt")
        self.dtnew = float(self.dt_dev.cpu()[0])
