"""TEST INFRASTRUCTURE: a numpy restatement of the implicit part of two-fluid (ion-neutral) MHD as the reference
performs it -- THREE SEPARATE PASSES over the arrays, one function per pass, each written in the reference's order
with its parenthesisation and true divisions (src/ion-neutral/ion-neutral_tasks.cpp:160-184, :189-246, :250-289) --
and of the ImEx tables of src/driver/driver.cpp:163-273.  numpy's float64 operations are IEEE operations rounded
once, like the reference's CPU build, so the product's one-launch kernel has to agree bit for bit.

One deliberate difference from the reference, shared with the product: a slab s whose coefficient is exactly 0.0 is
skipped by imex_exp (the reference adds 0.0*ru[s], which changes at most the sign of a zero).

Arrays: ui (nmb, nvar_i, ncell), un (nmb, nvar_n, ncell), ru (nimp_stages, nmb, 8, ncell); any trailing shape in place
of ncell works.  IDN, IM1..IM3 = 0..3.
"""
import numpy as np

IDN, IM1, IM2, IM3 = 0, 1, 2, 3


def tables(integrator):
    """driver.cpp:163-273, the literals"""
    gam0, gam1, beta = [0.0]*4, [0.0]*4, [0.0]*4
    at = [[0.0]*4 for _ in range(4)]
    gamma = 0.0
    if integrator == "imex2":
        nimp, nexp = 3, 2
        gam0[0], gam1[0], beta[0] = 1.0, 0.0, 1.0
        gam0[1], gam1[1], beta[1] = 0.5, 0.5, 0.5
        at[0][0], at[0][1], at[0][2] = -1.0, 0.0, 0.0
        at[1][0], at[1][1], at[1][2] = 0.5, 0.0, 0.0
        at[2][0], at[2][1], at[2][2] = 0.0, 0.25, 0.25
        a_impl = 0.5
    elif integrator == "imex2+":
        nimp, nexp = 4, 3
        gamma = 1.707106781186547
        gam0[0], gam1[0], beta[0] = 1.0, 0.0, gamma
        gam0[1] = (2.0*gamma - 1.0)/(2.0*gamma*gamma)
        gam1[1] = (1.0 - (2.0*gamma - 1.0)/(2.0*gamma*gamma))
        beta[1] = 1.0/(2.0*gamma)
        gam0[2], gam1[2], beta[2] = 1.0, 0.0, 0.0
        at[2][2] = (1.0 - 2.0*gamma*gamma)/2.0/gamma
        a_impl = gamma
    elif integrator == "imex3":
        nimp, nexp = 4, 3
        gam0[0], gam1[0], beta[0] = 1.0, 0.0, 1.0
        gam0[1], gam1[1], beta[1] = 0.25, 0.75, 0.25
        gam0[2], gam1[2], beta[2] = 2.0/3.0, 1.0/3.0, 2.0/3.0
        a = 0.24169426078821
        b = 0.06042356519705
        e = 0.12915286960590
        at[0][0] = -2.0*a
        at[1][0] = a
        at[1][1] = 1.0 - 2.0*a
        at[2][0] = b
        at[2][1] = e - ((1.0 - a)/4.0)
        at[2][2] = 0.5 - b - e - 1.25*a
        at[3][0] = (-2.0/3.0)*b
        at[3][1] = (1.0 - 4.0*e)/6.0
        at[3][2] = (4.0*(b + e + a) - 1.0)/6.0
        at[3][3] = 2.0*(1.0 - a)/3.0
        a_impl = a
    else:
        raise ValueError(integrator)
    return dict(integrator=integrator, nimp_stages=nimp, nexp_stages=nexp, gam0=gam0, gam1=gam1, beta=beta, a_twid=at,
                a_impl=a_impl, gamma=gamma)


def imex_exp(ui, un, ru, a_twid, istage, dt):
    """pass 1, :160-184: add the stiff source of the earlier stages; s ascending, zero coefficients skipped"""
    if istage <= 1:
        return
    for s in range(0, istage - 1):
        adt = np.float64(a_twid[istage - 2][s])*np.float64(dt)
        if adt == 0.0:
            continue
        ui[:, IM1] += adt*ru[s, :, 0]
        ui[:, IM2] += adt*ru[s, :, 1]
        ui[:, IM3] += adt*ru[s, :, 2]
        un[:, IM1] += adt*ru[s, :, 3]
        un[:, IM2] += adt*ru[s, :, 4]
        un[:, IM3] += adt*ru[s, :, 5]
        ui[:, IDN] += adt*ru[s, :, 6]
        un[:, IDN] += adt*ru[s, :, 7]


def imp_coefficients(tab, istage, dt, drag, xi, alpha):
    """:194-203"""
    if istage < 3 and tab["integrator"] == "imex2+":
        return np.float64(0.0), np.float64(0.0), np.float64(0.0)
    f = np.float64
    return f(drag)*f(tab["a_impl"])*f(dt), f(xi)*f(tab["a_impl"])*f(dt), f(alpha)*f(tab["a_impl"])*f(dt)


def imex_imp(ui, un, gamma_adt, xi_adt, alpha_adt):
    """pass 2, :210-245: the analytic solution of the implicit difference equations"""
    rho_i = ui[:, IDN].copy()
    if alpha_adt > 0:
        d = (1./4./alpha_adt/alpha_adt + xi_adt/2./alpha_adt/alpha_adt
             + xi_adt*xi_adt/4./alpha_adt/alpha_adt + ui[:, IDN]/alpha_adt +
             xi_adt/alpha_adt*(ui[:, IDN] + un[:, IDN]))
        rho_i = -1./2./alpha_adt - xi_adt/2./alpha_adt + np.sqrt(d)
    rho_n = ui[:, IDN] + un[:, IDN] - rho_i
    ui[:, IDN] = rho_i
    un[:, IDN] = rho_n
    denom = 1.0 + gamma_adt*(rho_i + rho_n) + xi_adt + alpha_adt*rho_i
    for im in (IM1, IM2, IM3):
        sum_ = (ui[:, im] + un[:, im])
        u_i = (ui[:, im] + (gamma_adt*rho_i + xi_adt)*sum_)/denom
        u_n = sum_ - u_i
        ui[:, im] = u_i
        un[:, im] = u_n


def imex_rup(ui, un, ru, s, drag, xi, alpha):
    """pass 3, :258-288: R(U) of the state just solved for, into ru[s]"""
    drag, xi, alpha = np.float64(drag), np.float64(xi), np.float64(alpha)
    for c, im in enumerate((IM1, IM2, IM3)):
        ru[s, :, c] = (drag*(ui[:, IDN]*un[:, im] - un[:, IDN]*ui[:, im]) +
                       xi*un[:, im] - alpha*ui[:, IDN]*ui[:, im])
    for c, im in enumerate((IM1, IM2, IM3)):
        ru[s, :, 3 + c] = (drag*(un[:, IDN]*ui[:, im] - ui[:, IDN]*un[:, im]) -
                           xi*un[:, im] + alpha*ui[:, IDN]*ui[:, im])
    ru[s, :, 6] = xi*un[:, IDN] - alpha*ui[:, IDN]*ui[:, IDN]
    ru[s, :, 7] = -xi*un[:, IDN] + alpha*ui[:, IDN]*ui[:, IDN]


def imp_rk_update(ui, un, ru, tab, estage, dt, drag, xi=0.0, alpha=0.0):
    """IonNeutral::ImpRKUpdate, :144-292: the three passes, in place"""
    istage = estage + 2
    imex_exp(ui, un, ru, tab["a_twid"], istage, dt)
    if estage < tab["nexp_stages"]:
        g_adt, xi_adt, al_adt = imp_coefficients(tab, istage, dt, drag, xi, alpha)
        imex_imp(ui, un, g_adt, xi_adt, al_adt)
        imex_rup(ui, un, ru, istage - 1, drag, xi, alpha)


def cycle_no_flux(ui, un, tab, dt, drag, xi=0.0, alpha=0.0):
    """one cycle of the two-fluid task list where the flux divergence of both fluids vanishes (a single cell, or a
    uniform periodic box): FirstTwoImpRK (copy, ImpRKUpdate(-1), ImpRKUpdate(0)), then per explicit stage the
    combination u0 = gam0*u0 + gam1*u1 - beta_dt*divF with divF = 0 (hydro_update.cpp:23-83) and ImpRKUpdate(stage).
    ui, un are updated in place; returns ru."""
    ru = np.zeros((tab["nimp_stages"], ui.shape[0], 8) + ui.shape[2:])
    ui1, un1 = ui.copy(), un.copy()
    imp_rk_update(ui, un, ru, tab, -1, dt, drag, xi, alpha)
    imp_rk_update(ui, un, ru, tab, 0, dt, drag, xi, alpha)
    for stage in range(1, tab["nexp_stages"] + 1):
        gam0, gam1 = np.float64(tab["gam0"][stage - 1]), np.float64(tab["gam1"][stage - 1])
        beta_dt = np.float64(tab["beta"][stage - 1])*np.float64(dt)
        ui[...] = gam0*ui + gam1*ui1 - beta_dt*0.0
        un[...] = gam0*un + gam1*un1 - beta_dt*0.0
        imp_rk_update(ui, un, ru, tab, stage, dt, drag, xi, alpha)
    return ru
