"""units::Units -- code scales in cgs, <units> (src/units/units.hpp, units.cpp).

Created by MeshBlockPack::AddPhysics iff the deck holds a <units> block (meshblock_pack.cpp:108-112).  The
derived scales are written with the reference's expressions in its order of operations: they enter the cooling
rate of <*_srcterms>/ism_cooling, so another association would change its bits.  The branch of the reference's
constructor that derives the scales from a black-hole mass (<coord>/general_rel = true) is refused: there is no
general relativity on this path.  csrc/akmi_host.cpp holds the same expressions for the C++ host.
"""

# cgs constants of units.hpp:28-49 (the ones used here)
atomic_mass_unit_cgs = 1.660538921e-24    # g
k_boltzmann_cgs = 1.3806488e-16           # erg/K


class Units:
    atomic_mass_unit_cgs = atomic_mass_unit_cgs
    k_boltzmann_cgs = k_boltzmann_cgs

    def __init__(self, pin):
        self.length_cgs_ = pin.GetOrAddReal("units", "length_cgs", 1.0)
        self.mass_cgs_ = pin.GetOrAddReal("units", "mass_cgs", 1.0)
        self.time_cgs_ = pin.GetOrAddReal("units", "time_cgs", 1.0)
        self.mu_ = pin.GetOrAddReal("units", "mu", 1.0)
        if pin.GetOrAddBoolean("coord", "general_rel", False):
            raise RuntimeError("### FATAL ERROR <units> from a black-hole mass (<coord>/general_rel = true) is not "
                               "on this path")

    def length_cgs(self):
        return self.length_cgs_

    def mass_cgs(self):
        return self.mass_cgs_

    def time_cgs(self):
        return self.time_cgs_

    def mu(self):
        return self.mu_

    def velocity_cgs(self):
        return self.length_cgs()/self.time_cgs()

    def density_cgs(self):
        return self.mass_cgs()/(self.length_cgs()*self.length_cgs()*self.length_cgs())

    def energy_cgs(self):
        return self.mass_cgs()*self.velocity_cgs()*self.velocity_cgs()

    def pressure_cgs(self):
        return self.energy_cgs()/(self.length_cgs()*self.length_cgs()*self.length_cgs())

    def temperature_cgs(self):
        return (self.velocity_cgs()*self.velocity_cgs()*self.mu()*self.atomic_mass_unit_cgs
                / self.k_boltzmann_cgs)
