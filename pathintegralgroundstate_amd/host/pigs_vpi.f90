!-----------------------------------------------------------------------
! pigs_vpi -- the vpi.in-driven front end on MI355X.
!
!   pigs_vpi < vpi.in
!
! Reads the reference's six namelists from standard input (system, samp, obdm, wavefun,
! extpot, jastrow -- same names, same defaults, reference vpi_mod.f90:14-80,
! system_mod.f90:15-34) plus one optional group of its own,
!     &gpu  n_walkers = 1, device = 0, n_gpus = 1, [device_sampler = T|F,] potential = 'aziz2', k1_variant = 0  /
! (n_gpus = G: the walkers are sharded in contiguous blocks over G GPUs -- devices device .. device+G-1, one
! context and one OpenMP host thread per GPU, no exchange while sampling -- and the block estimators of the shards
! meet ONCE per block in one all-reduce (RCCL over xGMI: pigs_comm_init_all / pigs_estimators_allreduce); thread 0
! writes the walker-summed files.  same_device = T puts every shard on `device`: a one-GPU rehearsal.)
! (potential: aziz2 | lj | dipolar -- the reference selects it by editing system_mod.f90)
! (density_profile = T, trapped systems only: the planar and radial density and the pair distribution of the middle
! slice, accumulated on the GPU -- dens_vpi.out, rho_vpi.out, pr_vpi.out; grid half-width rcut/2, Nbin bins per axis)
! (fq_tau = T, periodic systems only: the imaginary-time density correlations F(q,tau_l) = <rho_q(tau0+tau_l) rho_-q(tau0)>/Np
! on the S(k) grid for the lags l = 0..fq_ntau (tau_l = l dt) between the slices Nb-fq_window..Nb+fq_window, accumulated
! on the GPU -- fqt_vpi.out; fq_window defaults to ceiling(fq_ntau/2) and must stay inside the part of the path where
! the projection has converged: that is the user's choice, the program does not judge it)
! (sq_vector = T, periodic systems only: the structure factor S(q) on the full reciprocal grid, all integer vectors
! |n_k| <= sq_nmax (default 8) of the half space, averaged over the slices Nb-sq_window..Nb+sq_window (default 0),
! accumulated on the GPU -- sqvec_vpi.out, one line per vector, and sq_vpi.out, one line per |q| shell)
! (gr_vector = T, periodic systems only: the pair distribution g(r) on the Cartesian grid of the minimum-image cell,
! gr_nbin bins per axis (default 32), and radially on the run's own Nbin/rbin grid, both averaged over the slices
! Nb-gr_window..Nb+gr_window (default 0), accumulated on the GPU -- grvec_vpi.out, one line per bin, and grw_vpi.out in
! gr_vpi.out's format)
! (fq_vector = T, periodic systems only: F(q,tau_l) on the full reciprocal grid, the vectors of sq_vector with |n_k| <=
! fqv_nmax (default 8), for the lags l = 0..fqv_ntau (default 0) between the slices Nb-fqv_window..Nb+fqv_window (default
! ceiling(fqv_ntau/2)), accumulated on the GPU -- fqvec_vpi.out, one line per (lag, vector), and fqsh_vpi.out, one line
! per (lag, |q| shell))
! (fq_self = T, periodic systems only: the self (incoherent) part F_s(q,tau_l) on the vectors |n_k| <= fqs_nmax (default 8)
! and the imaginary-time mean-square displacement <|x_i(tau_l) - x_i(0)|^2>, for the lags l = 0..fqs_ntau (default 0)
! between the slices Nb-fqs_window..Nb+fqs_window (default ceiling(fqs_ntau/2)), accumulated on the GPU for the
! diagonal-sector walkers of a step -- fqself_vpi.out, one line per (lag, vector), fqssh_vpi.out, one line per (lag, |q|
! shell), and msd_vpi.out, one line per lag: l, tau_l, <dr^2>, error, alpha_2; the displacement is folded once, so it is
! the true one while it stays below half the box)
! (tau_profile = T, periodic and trapped systems: the imaginary-time profiles of every slice b = 0..2Nb -- pair and external
! potential energy, the virial W = sum r v'(r) and the kinetic estimator of every link, per particle, accumulated on the
! GPU -- tau_vpi.out; the plateau of V(tau) around slice Nb is the converged part of the path, in which the windows above
! must stay.  Periodic runs also write press_vpi.out, the virial pressure per block with W averaged over the slices
! Nb-tau_window..Nb+tau_window (default 0); W stops at rcut and no tail correction is made)
! (bond_order = T, periodic systems in 2D and 3D only: the bond-orientational order over the slices
! Nb-bo_window..Nb+bo_window (default 0), bonds being the pairs closer than bo_rnb (required, at most half the shortest
! side of the box), accumulated on the GPU -- bo_vpi.out, one line: Q4, Q6, the particle means of q4(i), q6(i) and the
! coordination, each with its error (2D: Psi4, Psi6, |psi4(i)|, |psi6(i)|); boh_vpi.out, one line per bin of bo_nhist
! (default 50) over [0,1]: centre, P(q4), P(q6) with their errors; g6_vpi.out: r and G6(r) on bo_nr bins of width
! rcut/bo_nr (default: the run's Nbin and rbin) in gr_vpi.out's format, bins without pairs in a block counting as 0)
! (van_hove = T, periodic systems only: the van Hove functions for the lags tau_l = l*dt, l = 0..vh_ntau, between the slices
! Nb-vh_window..Nb+vh_window (vh_window left out: the smallest window that holds the lags), accumulated on the GPU --
! gd_vpi.out: the distinct part G_d(r,tau), the histogram of |x_i(tau0+tau) - x_j(tau0)| over i /= j on the run's own
! Nbin/rbin grid, normalised like gr_vpi.out (lag 0 IS g(r)); gs_vpi.out: the self part G_s(r,tau), the probability
! density of the displacement |x_i(tau0+tau) - x_i(tau0)| on vh_nself bins (default 50) over [0, vh_rself) (default
! rcut); both one line per (lag, bin): tau_l, r, G and its error)
! (triplet = T, periodic systems in 2D and 3D only: the triplet distribution over the slices Nb-g3_window..Nb+g3_window
! (default 0), accumulated on the GPU: for every vertex the pairs of its legs, the partners closer than g3_rmax (left out
! or <= 0: rcut; at most half the shortest side), on g3_nr radial bins (default 10) and g3_na bins of cos(theta) (default
! 20) -- g3_vpi.out, one line per (lo, hi, q) with the leg bins lo <= hi: r_lo, r_hi, cos(theta), g3 and its error,
! normalised to 1 for an uncorrelated system; g3ang_vpi.out: cos(theta), the bond-angle distribution P(cos theta) of the
! legs below g3_rmax, which integrates to 1, and its error)
! (three_body = T, periodic systems in 2D and 3D only: the Axilrod-Teller-Muto (triple-dipole) energy, evaluated on the GPU on
! the sampled configurations over the slices Nb-atm_window..Nb+atm_window (default 0): the sum over the triplets i < j < k
! whose three nearest-image sides all lie within atm_rc (left out or <= 0: half the shortest side) of
! nu (1 + 3 cos cos cos)/(r_ij r_ik r_jk)^3, with the coupling atm_nu in the run's own units (energy length^9; left out: 1,
! the bare geometric sum) -- v3_vpi.out, one line per block: the block, V3/Np over the window, and its pressure
! P3 = 9 density (V3/Np)/dim (cut at atm_rc, no tail correction); v3tau_vpi.out, one line per window slice: a,
! tau_a = (a-Nb) dt, V3/Np and its error, the mean number of triplets)
! (momentum = T, periodic systems with CWorm > 0 only: the momentum distribution on the box-commensurate vectors
! |n_k| <= nk_nmax (default 8) from the end-to-end vectors of the open worldlines, every sample of the OBDM histogram and
! those beyond rcut too, and the one-body density matrix on nk_nbin (default 32) bins per axis of the minimum-image cell,
! normalised with nr_vpi.out's zconf in the blocks that normalise nr_vpi.out -- nkvec_vpi.out, one line per vector (n = 0
! first): n_1..n_dim, |k|, n(k), error; nk_vpi.out, one line per |k| shell; n0_vpi.out, one line per block: block, n0,
! n(k=0); nrvec_vpi.out, one line per bin: the bin centre, rho1/density, error)
! (lattice = T, periodic systems in 2D and 3D only: a crystal seen from the lattice sites, the coordinate lines of
! config_ini.in (their number is its first line and need not be Np), over the slices Nb-lat_window..Nb+lat_window (default 0):
! every particle is assigned to its nearest site on the GPU; lat_cm = T (default) removes the mean displacement of every
! slice; lat_nbin bins (default Nbin) up to lat_rmax (default half the sites' nearest-neighbour distance) -- lind_vpi.out,
! one line per block: the block, <u^2>, the Lindemann ratio, alpha_2, the vacant and the multiply occupied fraction of the
! sites, hops per particle and link, hops per particle across the window; lindtau_vpi.out, one line per window slice: tau,
! <u^2>, <u_k^2>, gamma; usite_vpi.out, one line per bin: r, rho_site(r), P(u_k = -r) and P(u_k = +r) per axis)
! (superfluid = T, periodic systems only: the superfluid fraction at T = 0 from the diffusion of the centre of mass along
! imaginary time, every link folded once and the folded links added up on the GPU, over the lags 0..sf_ntau (default 0)
! between the slices Nb-sf_window..Nb+sf_window (default: the smallest window that holds the lags) -- rhos_vpi.out, one line
! per lag l >= 1: tau, then value and error of Dcm per axis, of rhos = Dcm/(2 lambda tau) per axis (lambda = 1/2) and of
! their mean; msdu_vpi.out, one line per lag: tau, then value and error of the unfolded <dx_k^2> per axis, of their sum and
! of the cross term Dcm - <dx_k^2> per axis)
! (clusters = T, periodic systems only: the connected components of the bond graph r_ij < cl_rc (minimum image; left out or
! <= 0: rcut; at most half the shortest side) of every slice Nb-cl_window..Nb+cl_window (default 0), labelled on the GPU --
! clus_vpi.out, one line per cluster size s that occurred: s, then value and error over the blocks of n(s), the clusters of
! size s per slice, of the particle fraction s n(s)/Np and of P_largest(s), then <Rg^2>(s) = <sum of Rg^2 per slice> / <n(s)>
! and the error of its numerator over <n(s)>; clusblk_vpi.out, one line per block: the block, clusters per slice, <largest
! cluster>/Np, the mean cluster size sum s^2 n(s) / sum s n(s), bonds per particle)
! (percolation = T, periodic systems only: the clusters of the bond graph r_ij < pc_rc (as clusters = T has them; left out
! or <= 0: rcut) of every slice Nb-pc_window..Nb+pc_window that wrap the box, the finite ones and their unfolded extent,
! and the persistence of clusters over the lags 0..pc_ntau (default 0; pc_window left out: the smallest window that holds
! the lags) -- perc_vpi.out, one line per block: the block, the share of the slices with a cluster that wraps along x, y,
! z (0 beyond dim), along any axis, along all axes, the strength P_inf (the share of the particles in wrapping clusters)
! and the mean finite cluster size; percsz_vpi.out, one line per finite cluster size s that occurred: s, value and error
! of n_fin(s)/Np, then <Rg^2>(s) from unfolded separations as a ratio of two block means and the error of its numerator
! over the denominator; clpers_vpi.out, one line per lag l: l, tau, value and error of the pairs per origin that share a
! cluster in slice a, in a+l and in both, the persistence <both>/<first> and the Jaccard index)
! (device_sampler = T: the whole MC step of every walker runs on the GPU in one launch, kernel K6 -- every mover of
! the reference; F: the host-driven lock-step sampler, one K1 batch per move stage.  Left out: K6 wherever it serves
! the input, the host-driven sampler otherwise.  The two give the same files and the same worldlines, bit for bit.)
! runs n_walkers independent PIGS chains in lock-step (walker w uses seed+w-1, so walker 1
! IS the reference's chain), every Delta S / energy sum on the GPU through libpigs_hip.so,
! and writes the reference's observable files: e_vpi.out, et_vpi.out ('(5g20.10e3)'),
! gr_vpi.out, sk_vpi.out, nr_vpi.out ('(20g20.10e3)'), fort.99-style permutation histogram
! (perm_vpi.out), plus e_vpi.hex / et_vpi.hex with the same numbers as 64-bit hex for
! parity checks beyond 10 digits.  With n_walkers > 1 the per-walker files carry a .wNNNN
! suffix and the unsuffixed files hold the walker average.
! The step / block structure follows reference vpi.f90:244-588.
!-----------------------------------------------------------------------
program pigs_vpi

  use iso_c_binding
  use pigs_capi
  use pigs_rng
  use pigs_sampler
  use pigs_estimators
  use pigs_families
  use pigs_shard
  use omp_lib

  implicit none

  ! ---- namelist variables (names fixed by the input format)
  logical           :: crystal,trap,resume,swapping,wf_table,v_table
  character (len=3) :: sampling
  real (kind=8)     :: density,dt,delta_cm,CWorm,Rm
  real (kind=8)     :: a_ho(3)
  integer           :: dim,Np,Nb,seed,CMFreq,Lstag,Nlev,Nstag,Nblock,Nstep,Nbin,Nk
  integer           :: Nobdm,Npw,Nmax,n_walkers,device,ios,k1_variant,n_gpus
  logical           :: device_sampler,checkpointing,same_device,density_profile,fq_tau
  integer           :: fq_ntau,fq_window
  logical           :: sq_vector
  integer           :: sq_nmax,sq_window
  logical           :: gr_vector
  integer           :: gr_nbin,gr_window
  logical           :: fq_vector
  integer           :: fqv_nmax,fqv_ntau,fqv_window
  logical           :: fq_self
  integer           :: fqs_nmax,fqs_ntau,fqs_window
  logical           :: tau_profile
  integer           :: tau_window
  logical           :: bond_order
  real (kind=8)     :: bo_rnb
  integer           :: bo_nhist,bo_nr,bo_window
  logical           :: van_hove
  integer           :: vh_ntau,vh_window,vh_nself
  real (kind=8)     :: vh_rself
  logical           :: triplet
  integer           :: g3_nr,g3_na,g3_window
  real (kind=8)     :: g3_rmax
  logical           :: three_body
  integer           :: atm_window
  real (kind=8)     :: atm_nu,atm_rc
  logical           :: momentum
  logical           :: lattice,lat_cm
  integer           :: lat_nbin,lat_window
  real (kind=8)     :: lat_rmax
  logical           :: superfluid
  integer           :: sf_ntau,sf_window
  logical           :: clusters
  real (kind=8)     :: cl_rc
  integer           :: cl_window
  logical           :: percolation
  real (kind=8)     :: pc_rc
  integer           :: pc_window,pc_ntau
  integer           :: nk_nmax,nk_nbin
  type(family_keys) :: fk                ! the estimator keys, as the families take them
  type(family_set)  :: keyed             ! (the main program's set checks the keys and prints the banner; every shard has its own)
  logical           :: sampler_auto
  integer(c_int)    :: rc_probe
  type(pigs_sweep_params) :: probe_par
  character (len=8) :: potential
  integer           :: pot_kind
  namelist /system/  dim,Np,density,crystal,trap
  namelist /samp/    resume,dt,Nb,seed,delta_cm,CMFreq,sampling,Lstag,Nlev,Nstag,Nblock,Nstep,Nbin,Nk
  namelist /obdm/    swapping,CWorm,Nobdm,Npw
  namelist /wavefun/ Nmax,wf_table,v_table
  namelist /extpot/  a_ho
  namelist /jastrow/ Rm
  namelist /gpu/     n_walkers,device,device_sampler,potential,checkpointing,k1_variant,n_gpus,same_device,density_profile, &
       &             fq_tau,fq_ntau,fq_window,sq_vector,sq_nmax,sq_window, &
       &             gr_vector,gr_nbin,gr_window, &
       &             fq_vector,fqv_nmax,fqv_ntau,fqv_window, &
       &             tau_profile,tau_window, &
       &             fq_self,fqs_nmax,fqs_ntau,fqs_window, &
       &             bond_order,bo_rnb,bo_nhist,bo_nr,bo_window, &
       &             van_hove,vh_ntau,vh_window,vh_nself,vh_rself, &
       &             triplet,g3_nr,g3_na,g3_rmax,g3_window, &
       &             three_body,atm_nu,atm_rc,atm_window, &
       &             momentum,nk_nmax,nk_nbin, &
       &             lattice,lat_nbin,lat_rmax,lat_window,lat_cm, &
       &             superfluid,sf_ntau,sf_window, &
       &             clusters,cl_rc,cl_window, &
       &             percolation,pc_rc,pc_window,pc_ntau


  ! shared by the shards (read-only once the parallel region starts)
  type(pigs_params)  :: gp
  type(c_ptr), allocatable :: ctxs(:)
  integer, allocatable :: lo(:),hi(:)
  real(8) :: Lbox(3),rcut,rcut2,rbin,dr,pi
  real(8), allocatable :: VTable(:),LogWF(:)
  integer :: NWtot,G,ish0,k,ucfg0
  real(8), allocatable :: chk_all(:,:,:,:),AE_all(:,:),AT_all(:,:)
  integer, allocatable :: diag_bl_all(:)

  !---------------------------------------------------------------------
  ! defaults (reference vpi_mod.f90:39-60) and input
  crystal = .false.; trap = .false.
  resume = .false.; seed = 1982; Lstag = 2; Nlev = 1
  swapping = .false.; CWorm = 0.d0; Nobdm = 0; Npw = 0
  Nmax = 10000; wf_table = .false.; v_table = .false.
  CMFreq = 1; Nstag = 1; Nblock = 1; Nstep = 1; Nbin = 100; Nk = 50; sampling = 'bis'
  delta_cm = 0.d0; density = 0.d0; a_ho = 1.d0; Rm = 1.d0
  n_walkers = 1; device = 0; device_sampler = .false.; potential = 'aziz2'; checkpointing = .true.; k1_variant = 0
  n_gpus = 1; same_device = .false.; density_profile = .false.
  fq_tau = .false.; fq_ntau = 0; fq_window = -1
  sq_vector = .false.; sq_nmax = 8; sq_window = 0
  gr_vector = .false.; gr_nbin = 32; gr_window = 0
  fq_vector = .false.; fqv_nmax = 8; fqv_ntau = 0; fqv_window = -1
  tau_profile = .false.; tau_window = 0
  fq_self = .false.; fqs_nmax = 8; fqs_ntau = 0; fqs_window = -1
  bond_order = .false.; bo_rnb = 0.d0; bo_nhist = 50; bo_nr = -1; bo_window = 0
  van_hove = .false.; vh_ntau = 0; vh_window = -1; vh_nself = 50; vh_rself = 0.d0
  triplet = .false.; g3_nr = 10; g3_na = 20; g3_rmax = 0.d0; g3_window = -1
  momentum = .false.; nk_nmax = 8; nk_nbin = 32
  lattice = .false.; lat_nbin = 0; lat_rmax = 0.d0; lat_window = -1; lat_cm = .true.
  superfluid = .false.; sf_ntau = 0; sf_window = -1
  clusters = .false.; cl_rc = 0.d0; cl_window = -1
  percolation = .false.; pc_rc = 0.d0; pc_window = -1; pc_ntau = 0
  three_body = .false.; atm_nu = -huge(1.d0); atm_rc = 0.d0; atm_window = -1        ! (atm_nu: a value nobody gives, left out -> 1)

  read (5,nml=system,iostat=ios);  rewind (5)
  read (5,nml=samp,iostat=ios);    rewind (5)
  read (5,nml=obdm,iostat=ios);    rewind (5)
  read (5,nml=wavefun,iostat=ios); rewind (5)
  if (trap) then
     read (5,nml=extpot,iostat=ios); rewind (5)
  end if
  read (5,nml=jastrow,iostat=ios); rewind (5)
  ! device_sampler left out of &gpu = automatic: the device-resident sampler (K6) wherever it serves the input, the
  ! host-driven one otherwise.  Whether it was given is found by reading the group twice with opposite defaults.
  device_sampler = .true.
  read (5,nml=gpu,iostat=ios);     rewind (5)
  sampler_auto = device_sampler
  device_sampler = .false.
  read (5,nml=gpu,iostat=ios);     rewind (5)
  sampler_auto = sampler_auto .neqv. device_sampler

  if (.not. v_table) then
     write (0,*) 'pigs_vpi: v_table = T is required (the reference Force() is a stub: system_mod.f90:186-209)'
     stop 2
  end if
  NWtot = n_walkers
  G = max(1,min(n_gpus,NWtot))
  pi = acos(-1.d0)
  if (Lstag>Nb .and. CWorm>0.d0) then
     ! the worm-sector movers cut segments of up to Lstag beads out of a HALF chain: beyond Nb the reference indexes
     ! Path below bead 0 / above bead 2Nb (vpi_mod.f90:1853-1857, 2112-2116, 2300) and may even accept what it read
     ! there.  With CWorm = 0 the open proposal is never accepted (quirk Q11) and both samplers only draw its
     ! random numbers; with CWorm > 0 there is no defined result to reproduce: refuse the input.
     write (0,*) 'pigs_vpi: CWorm > 0 needs Lstag <= Nb (worm moves act on half chains of Nb links)'
     stop 2
  end if

  ! box, cutoff, grids (reference vpi.f90:82-128)
  Lbox = 1.d0
  if (trap) then
     rcut = 1.d0
     do k=1,dim
        rcut = 3.d0*rcut*a_ho(k)
     end do
     density  = real(Np)/(pi**(0.5d0*dim)*rcut/gamma(0.5d0*dim+1.d0))
     rcut     = rcut**(1.d0/real(dim))
     rcut     = 10.d0*rcut
     delta_cm = delta_cm*minval(a_ho(1:dim))
  else
     if (crystal) then
        ! lattice start: particle number, box and density come from config_ini.in (reference vpi.f90:99-107)
        open (newunit=ucfg0,file='config_ini.in',status='old')
        read (ucfg0,*) Np
        read (ucfg0,*) (Lbox(k),k=1,dim)
        read (ucfg0,*) density
        close (ucfg0)
     else
        do k=1,dim
           Lbox(k) = (real(Np)/density)**(1.d0/real(dim))
        end do
     end if
     rcut     = minval(0.5d0*Lbox(1:dim))
     delta_cm = delta_cm/density**(1.d0/real(dim))
  end if
  rcut2 = rcut*rcut
  rbin  = rcut/real(Nbin)

  ! the estimator keys: refused values end the run before the backend is asked for the key's entry points
  ! (after the box: bo_rnb is measured against half its shortest side, which is rcut in a periodic system)
  fk = family_keys(density_profile=density_profile,fq_tau=fq_tau,fq_ntau=fq_ntau,fq_window=fq_window, &
       & sq_vector=sq_vector,sq_nmax=sq_nmax,sq_window=sq_window,gr_vector=gr_vector,gr_nbin=gr_nbin,gr_window=gr_window, &
       & fq_vector=fq_vector,fqv_nmax=fqv_nmax,fqv_ntau=fqv_ntau,fqv_window=fqv_window,tau_profile=tau_profile, &
       & tau_window=tau_window,fq_self=fq_self,fqs_nmax=fqs_nmax,fqs_ntau=fqs_ntau,fqs_window=fqs_window, &
       & bond_order=bond_order,bo_rnb=bo_rnb,bo_nhist=bo_nhist,bo_nr=bo_nr,bo_window=bo_window,half_side=rcut, &
       & van_hove=van_hove,vh_ntau=vh_ntau,vh_window=vh_window,vh_nself=vh_nself,vh_rself=vh_rself, &
       & triplet=triplet,g3_nr=g3_nr,g3_na=g3_na,g3_rmax=g3_rmax,g3_window=g3_window, &
       & three_body=three_body,atm_nu_given=atm_nu/=-huge(1.d0),atm_nu=merge(atm_nu,1.d0,atm_nu/=-huge(1.d0)), &
       & atm_rc=atm_rc,atm_window=atm_window, &
       & momentum=momentum,nk_nmax=nk_nmax,nk_nbin=nk_nbin,cworm=CWorm,nobdm=Nobdm, &
       & lattice=lattice,lat_nbin=lat_nbin,lat_rmax=lat_rmax,lat_window=lat_window,lat_cm=lat_cm,nbin_run=Nbin,box=Lbox, &
       & superfluid=superfluid,sf_ntau=sf_ntau,sf_window=sf_window, &
       & clusters=clusters,cl_rc=cl_rc,cl_window=cl_window, &
       & percolation=percolation,pc_rc=pc_rc,pc_window=pc_window,pc_ntau=pc_ntau)
  call keyed%create(fk)
  call keyed%check(fk,dim,Nb,trap)

  ! tables on the host (reference vpi_mod.f90:84-145), then the GPU context
  allocate (VTable(0:Nmax+1),LogWF(0:Nmax+1))
  ! the reference picks its pair potential by editing system_mod.f90; here it is an input
  select case (trim(potential))
  case ('aziz2');   pot_kind = 0
  case ('lj');      pot_kind = 1
  case ('dipolar'); pot_kind = 2
  case default
     write (0,*) 'pigs_vpi: unknown potential ',trim(potential),' (aziz2 | lj | dipolar)'
     stop 2
  end select
  call pigs_check(pigs_build_tables_kind(int(pot_kind,c_int32_t),int(Nmax,c_int32_t),Rm,rcut,VTable,LogWF,dr), &
       & 'pigs_build_tables_kind')
  gp%dim = dim; gp%Np = Np; gp%Nb = Nb; gp%Nmax = Nmax
  gp%trap = merge(1,0,trap); gp%wf_table = merge(1,0,wf_table); gp%v_table = 1; gp%reserved = 0
  gp%dr = dr; gp%rcut2 = rcut2; gp%dt = dt; gp%Rm = Rm
  gp%Lbox = Lbox; gp%a_ho = a_ho
  ! one context per GPU, each with a contiguous block of walkers (sharding.shard_walkers: the first mod(NW,G) shards
  ! get one walker more); walker w (global, 1-based) runs the chain of seed+w-1 whatever the partition
  allocate (ctxs(G),lo(G),hi(G))
  do ish0=1,G
     lo(ish0) = (ish0-1)*(NWtot/G)+min(ish0-1,mod(NWtot,G))+1
     hi(ish0) = lo(ish0)+NWtot/G-1
     if (ish0<=mod(NWtot,G)) hi(ish0) = hi(ish0)+1
     call pigs_check(pigs_ctx_create(gp,VTable,LogWF,int(hi(ish0)-lo(ish0)+1,c_int32_t), &
          & int(merge(device,device+ish0-1,same_device),c_int32_t),ctxs(ish0)),'pigs_ctx_create')
     ! k1_variant = 2 selects the Delta-S kernel that keeps the reference's rounding of every term (default 0: short arithmetic)
     if (k1_variant/=0) call pigs_check(pigs_set_tuning(ctxs(ish0),'k1_variant'//c_null_char,int(k1_variant,c_int32_t)), &
          & 'pigs_set_tuning')
  end do
  if (G>1) call pigs_check(pigs_comm_init_all(ctxs,int(G,c_int32_t)),'pigs_comm_init_all')
  if (sampler_auto) then
     ! both samplers give the same files and the same worldlines, bit for bit (soaked against each other and against the
     ! reference's arithmetic: profiles/r03_k6_vs_host_soak.txt); the device-resident one is ~30 times faster at N = 256
     call fill_sweep_params(probe_par)
     rc_probe = pigs_sampler_init(ctxs(1),probe_par)
     device_sampler = rc_probe==PIGS_OK
  end if
  allocate (chk_all(dim,Np,0:2*Nb,NWtot),AE_all(3,NWtot),AT_all(3,NWtot),diag_bl_all(NWtot))
  diag_bl_all = 0

  print '(a)',       ' =============================================================='
  print '(a)',       '            VPI Monte Carlo on MI355X (pigs_vpi)               '
  print '(a)',       ' =============================================================='
  print '(a,i6)',    '  > Walkers (lock-step) :',NWtot
  print '(a,i6)',    '  > GPUs (walker shards):',G
  print '(a,i6)',    '  > Dimensions          :',dim
  print '(a,i6)',    '  > Number of particles :',Np
  print '(a,i6)',    '  > Number of beads     :',Nb
  print '(a,g13.6)', '  > Time step           :',dt
  print '(a,i6)',    '  > Number of blocks    :',Nblock
  print '(a,i6)',    '  > MC steps per block  :',Nstep
  if (device_sampler) then
     print '(a)',    '  > Sampler             : device-resident (K6: one launch per MC step)'
  else if (sampler_auto) then
     print '(a)',    '  > Sampler             : host-driven (the device-resident sampler does not serve this input or backend)'
  else
     print '(a)',    '  > Sampler             : host-driven (lock-step batches through K1)'
  end if
  call keyed%banner(fk,trap)

  !=====================================================================

  !$omp parallel num_threads(G) default(shared)
  call run_shard(omp_get_thread_num()+1)
  !$omp end parallel

  print '(a)', ' =============================================================='
  print '(a)', ' FINAL RESULTS (per walker: <E> <Ec> <Ep> | <Et> <Kt> <Vt>, per particle)'
  do k=1,NWtot
     if (diag_bl_all(k)>0) print '(i6,6g16.8)', k-1,AE_all(:,k)/real(diag_bl_all(k))/Np,AT_all(:,k)/real(diag_bl_all(k))/Np
  end do
  print '(a)', ' =============================================================='
  open (newunit=k,file='worldlines_final.bin',form='unformatted',access='stream')
  write (k) chk_all
  close (k)
  do ish0=1,G
     call pigs_check(pigs_ctx_destroy(ctxs(ish0)),'pigs_ctx_destroy')
  end do

contains

  ! namelists samp + obdm as the library's sweep parameters
  subroutine fill_sweep_params(p)
    type(pigs_sweep_params), intent(out) :: p
    p%Nlev = Nlev; p%Nstag = Nstag; p%CMFreq = CMFreq; p%Lstag = Lstag
    p%delta_cm = delta_cm
    p%CWorm = CWorm; p%density = density; p%rbin = rbin
    p%sampling = merge(1,0,sampling=="sta")
    p%swapping = merge(1,0,swapping); p%Nobdm = Nobdm; p%Nbin = Nbin; p%Npw = Npw
    p%reserved = 0
  end subroutine fill_sweep_params

  ! initial configuration of the shard's walkers w0+1.. (reference vpi_mod.f90:149-259): resume from checkpoint files, a
  ! lattice from config_ini.in, or uniform random positions; every bead of a particle starts at the same point; walker w
  ! seeds its stream with seed+w-1
  subroutine initial_configuration(s,w0)
    type(sampler_t), intent(inout) :: s
    integer, intent(in) :: w0
    integer :: w,k,ip,ib,j,ucfg
    logical :: lflag
    character(len=32) :: suffix
    do w=1,s%W
       suffix = walker_suffix(w0+w-1)
       if (resume) then
          open (newunit=ucfg,file='checkpoint'//trim(suffix)//'.dat',status='old')
          read (ucfg,*) lflag                      ! trap: the reference's init takes it from the file (vpi_mod.f90:166);
          if (lflag .neqv. trap) then              ! here the tables and the box were already built from the namelist value,
             write (0,*) 'pigs_vpi: checkpoint',trim(suffix),'.dat was written with trap = ',lflag, &   ! so a mismatch is an error
                  & ' but the namelist says trap = ',trap
             stop 2
          end if
          read (ucfg,*) lflag
          s%isopen(w) = lflag
          read (ucfg,*) s%iworm(w)
          do ip=1,Np
             do ib=0,2*Nb
                read (ucfg,*) (s%Path(k,ip,ib,w),k=1,dim)
             end do
          end do
          read (ucfg,*)
          read (ucfg,*)
          do j=1,2
             read (ucfg,*) (s%xend(k,j,w),k=1,dim)
          end do
          close (ucfg)
          call mt_load(s%rng(w),'rand_state'//trim(suffix))
          cycle
       end if
       call mt_seed(s%rng(w),seed+w0+w-1)
       if (crystal .and. .not. trap) then
          ! one shard at a time: the shards are threads of one process, and a file may be connected to one unit only
          !$omp critical (config_ini)
          open (newunit=ucfg,file='config_ini.in',status='old')
          read (ucfg,*)
          read (ucfg,*)
          read (ucfg,*)
          do ip=1,Np
             read (ucfg,*) (s%Path(k,ip,0,w),k=1,dim)
          end do
          close (ucfg)
          !$omp end critical (config_ini)
       else
          do ip=1,Np
             do k=1,dim
                if (trap) then
                   s%Path(k,ip,0,w) = 2.d0*a_ho(k)*(mt_real(s%rng(w))-0.5d0)
                else
                   s%Path(k,ip,0,w) = Lbox(k)*(mt_real(s%rng(w))-0.5d0)
                end if
             end do
          end do
       end if
       do ib=1,2*Nb
          s%Path(:,:,ib,w) = s%Path(:,:,0,w)
       end do
       s%xend(:,1,w) = s%Path(:,Np,Nb,w)
       s%xend(:,2,w) = s%xend(:,1,w)
    end do
  end subroutine initial_configuration

  ! checkpoint of the shard's walkers (reference vpi.f90:541-545, vpi_mod.f90:263-309): text worldline, particle-major
  subroutine write_checkpoints(s,w0)
    type(sampler_t), intent(in) :: s
    integer, intent(in) :: w0
    integer :: w,k,ip,ib,j,ucfg
    character(len=32) :: suffix
    do w=1,s%W
       suffix = walker_suffix(w0+w-1)
       open (newunit=ucfg,file='checkpoint'//trim(suffix)//'.dat')
       if (trap) then
          write (ucfg,*) ".True."
       else
          write (ucfg,*) ".False."
       end if
       if (s%isopen(w)) then
          write (ucfg,*) ".True."
       else
          write (ucfg,*) ".False."
       end if
       write (ucfg,*) s%iworm(w)
       do ip=1,Np
          do ib=0,2*Nb
             write (ucfg,*) (s%Path(k,ip,ib,w),k=1,dim)
          end do
       end do
       write (ucfg,*)
       write (ucfg,*)
       do j=1,2
          write (ucfg,*) (s%xend(k,j,w),k=1,dim)
       end do
       close (ucfg)
       call mt_save(s%rng(w),'rand_state'//trim(suffix))
    end do
  end subroutine write_checkpoints

  !---------------------------------------------------------------------
  ! one shard: the walkers lo(ish)..hi(ish) on context ctxs(ish), the reference's block / step structure
  ! (vpi.f90:244-588) for all of them in lock-step, one line per phase.  The shard's state (pigs_shard) is a local of this
  ! procedure and so private to the calling thread.
  subroutine run_shard(ish)
    integer, intent(in) :: ish
    type(shard_state) :: sh
    integer    :: iblock,istep
    integer(8) :: c0,c1,crate

    call shard_setup(sh,ish)
    do iblock=1,Nblock
       call system_clock(c0,crate)
       call sh%moves%reset()
       call sh%en%reset()
       call sh%core%reset()
       ! the estimators of a step are queued at its end and collected by the NEXT step (collect_estimators), those of the
       ! block's last step behind the loop
       do istep=1,Nstep
          if (device_sampler) then
             call step_device(sh,istep)
          else
             call step_host(sh,iblock,istep)
          end if
          call queue_estimators(sh)
       end do
       call collect_estimators(sh)
       call block_end(sh,iblock)
       if (checkpointing) call block_checkpoint(sh)
       call system_clock(c1)
       if (ish==1) call block_report(sh,iblock,dble(c1-c0)/dble(crate))
    end do
    call shard_finish(sh)
  end subroutine run_shard

  ! sampler, initial configuration, upload, the device-resident sampler's start state, block statistics, families, units
  subroutine shard_setup(sh,ish)
    type(shard_state), intent(inout) :: sh
    integer, intent(in) :: ish
    type(family_run)        :: frun
    type(pigs_sweep_params) :: swp_par
    integer(c_int32_t) :: nev
    character(len=8)   :: envbuf
    character(len=32)  :: suffix
    integer :: NW,w

    call get_environment_variable('PIGS_VPI_TRACE',envbuf)
    sh%trace = envbuf(1:1)=='1'
    NW = hi(ish)-lo(ish)+1
    sh%ish = ish; sh%NW = NW; sh%w0 = lo(ish)-1; sh%ctx = ctxs(ish)

    call sampler_init(sh%s,dim,Np,Nb,NW,trap,dt,density,CWorm,Lbox(1:dim),sh%ctx)
    if (ish==1 .and. .not. device_sampler) print '(a,i6)','  > host threads per stage:',sh%s%nthr
    sh%ep%dim = dim; sh%ep%Np = Np; sh%ep%Nbin = Nbin; sh%ep%Nk = Nk; sh%ep%Npw = Npw; sh%ep%trap = trap
    sh%ep%rcut2 = rcut2; sh%ep%rbin = rbin; sh%ep%pi = pi; sh%ep%CWorm = CWorm
    sh%ep%Lbox = Lbox; sh%ep%LboxHalf = 0.5d0*Lbox; sh%ep%qbin = 2.d0*pi/Lbox

    call initial_configuration(sh%s,sh%w0)
    call sampler_upload(sh%s)
    if (device_sampler) then
       call fill_sweep_params(swp_par)
       call pigs_check(pigs_sampler_init(sh%ctx,swp_par),'pigs_sampler_init')
       call pigs_check(pigs_sampler_event_ints(sh%ctx,nev),'pigs_sampler_event_ints')
       allocate (sh%dev%isopen(NW),sh%dev%iworm(NW),sh%dev%ev(nev,NW),sh%dev%nrho(0:Npw,Nbin,NW),sh%dev%reset(NW))
       sh%dev%isopen = merge(1,0,sh%s%isopen); sh%dev%iworm = sh%s%iworm
       call pigs_check(pigs_sampler_set_worm(sh%ctx,sh%dev%isopen,sh%dev%iworm,sh%s%xend),'pigs_sampler_set_worm')
       do w=1,NW
          call pigs_check(pigs_sampler_set_rng(sh%ctx,int(w-1,c_int32_t),int(sh%s%rng(w)%pos,c_int32_t),sh%s%rng(w)%w), &
               & 'pigs_sampler_set_rng')
       end do
       allocate (sh%pend%gr_inc(Nbin,NW),sh%pend%sk_inc(dim,Nk,NW),sh%dev%acc(NDEV_COUNTS,NW),sh%dev%acc0(NDEV_COUNTS,NW))
       sh%dev%acc0 = 0
    end if

    ! the first 20 doubles of the block vector: number of walkers with a diagonal block, their summed block energies, the
    ! block's counters; behind them the summed normalised g(r), S(k), n(r) and how many walkers contributed, then what the
    ! estimator keys add
    sh%nvec = 7+NSUMS
    call sh%core%create(sh%ep,density,Nobdm,NW,sh%nvec)
    frun%Nb = Nb; frun%dt = dt; frun%density = density; frun%rcut = rcut
    frun%averages = NWtot>1 .and. ish==1
    allocate (frun%suffix(NW))
    do w=1,NW
       frun%suffix(w) = walker_suffix(sh%w0+w-1)
    end do
    call sh%fams%create(fk)
    call sh%fams%setup(fk,frun,sh%ctx,sh%ep,NW,sh%nvec)
    allocate (sh%vec(sh%nvec))

    allocate (sh%perm(NW))
    do w=1,NW
       allocate (sh%perm(w)%members(Np),sh%perm(w)%histogram(Np))
       sh%perm(w)%members = 0; sh%perm(w)%histogram = 0
    end do
    allocate (sh%pend%en9(9,NW),sh%pend%list(NW))
    call sh%moves%create(NW)
    call sh%en%create(NW)

    allocate (sh%ue(NW),sh%ut(NW),sh%uh(NW))
    do w=1,NW
       suffix = walker_suffix(sh%w0+w-1)
       open (newunit=sh%ue(w),file='e_vpi'//trim(suffix)//'.out')
       open (newunit=sh%ut(w),file='et_vpi'//trim(suffix)//'.out')
       open (newunit=sh%uh(w),file='e_vpi'//trim(suffix)//'.hex')
    end do
    if (NWtot>1 .and. ish==1) then
       open (newunit=sh%ueav,file='e_vpi.out')
       open (newunit=sh%utav,file='et_vpi.out')
    end if
  end subroutine shard_setup

  ! one MC step of the host-driven sampler (reference vpi.f90:302-404), one K1 batch per move stage.  The previous step's
  ! estimators are collected first: the mirror still holds that step's worldlines, which g(r) and S(k) are taken from.
  subroutine step_host(sh,iblock,istep)
    type(shard_state), intent(inout) :: sh
    integer, intent(in) :: iblock,istep
    integer :: ipv(sh%NW),iupd(sh%NW),partner(sh%NW)
    logical :: act(sh%NW),isopen0(sh%NW),swp(sh%NW)
    integer :: w,ip,istag,iobdm,j

    call collect_estimators(sh)
    associate (s => sh%s, perm => sh%perm, n => sh%moves%n, try_cm => sh%moves%try_cm, try_stag => sh%moves%try_stag)
    ! ---- open / close attempt (reference vpi.f90:302-323)
    isopen0 = s%isopen
    do w=1,sh%NW
       iupd(w) = int(mt_real(s%rng(w))*2)
    end do
    act = isopen0 .and. iupd==0
    if (any(act)) then
       call mv_close(s,Lstag,act,n(:,ACC_CLOSE))
       do w=1,sh%NW
          if (.not. act(w)) cycle
          perm(w)%end_cycle = .not. s%isopen(w)
          n(w,TRY_CLOSE) = n(w,TRY_CLOSE)+1
          if (swapping) call perm_sampling(perm(w),s%isopen(w),s%iworm(w))
       end do
    end if
    act = (.not. isopen0) .and. iupd==1
    if (any(act)) then
       do w=1,sh%NW
          if (act(w)) s%iworm(w) = min(int(mt_real(s%rng(w))*Np)+1,Np)
       end do
       call mv_open(s,Lstag,s%iworm,act,n(:,ACC_OPEN))
       do w=1,sh%NW
          if (.not. act(w)) cycle
          perm(w)%new_cycle = s%isopen(w)
          n(w,TRY_OPEN) = n(w,TRY_OPEN)+1
          if (swapping) call perm_sampling(perm(w),s%isopen(w),s%iworm(w))
       end do
    end if

    ! ---- centre-of-mass and bead moves of every (non-worm) particle
    if (mod(istep,CMFreq)==0) then
       do ip=1,Np
          ipv = ip
          act = .not. (s%isopen .and. s%iworm==ip)
          where (act) try_cm = try_cm+1
          call mv_translate(s,delta_cm,ipv,act,n(:,ACC_CM))
       end do
    end if
    do istag=1,Nstag
       do ip=1,Np
          ipv = ip
          act = .not. (s%isopen .and. s%iworm==ip)
          where (act) try_stag = try_stag+1
          if (sampling=="sta") then
             call mv_end_staging(s,HEAD,Lstag,ipv,act,n(:,ACC_HEAD))
             call mv_end_staging(s,TAIL,Lstag,ipv,act,n(:,ACC_TAIL))
             call mv_staging(s,Lstag,ipv,act,n(:,ACC_BD))
          else
             call mv_end_bisection(s,HEAD,Nlev,ipv,act,n(:,ACC_HEAD))
             call mv_end_bisection(s,TAIL,Nlev,ipv,act,n(:,ACC_TAIL))
             call mv_bisection(s,Nlev,ipv,act,n(:,ACC_BD))
          end if
       end do
    end do

    ! ---- worm moves of the walkers in the off-diagonal sector (reference vpi.f90:370-404)
    act = s%isopen
    if (any(act)) then
       do iobdm=1,Nobdm
          do j=1,2
             call mv_translate_half(s,j,delta_cm,act,n(:,ACC_CM_HALF))
          end do
          do j=1,2
             call mv_end_staging_half(s,HEAD,j,Lstag,act,n(:,ACC_HEAD_HALF))
             call mv_end_staging_half(s,TAIL,j,Lstag,act,n(:,ACC_TAIL_HALF))
             call mv_staging_half(s,j,Lstag,act,n(:,ACC_BD_HALF))
          end do
          if (swapping) then
             where (act) n(:,TRY_SWAP) = n(:,TRY_SWAP)+1
             call mv_swap(s,Lstag,act,n(:,ACC_SWAP),partner,swp)
             do w=1,sh%NW
                if (act(w)) call perm_sampling(perm(w),s%isopen(w),s%iworm(w),partner(w),swp(w))
             end do
          end if
          if (.not. trap) then
             do w=1,sh%NW
                if (act(w)) call obdm_accumulate(sh%ep,s%xend(:,:,w),sh%core%nrho(:,:,w))
             end do
             call sh%fams%nk_add(sh%ctx,sh%NW,act,s%xend)
          end if
       end do
    end if
    if (sh%trace) then                    ! PIGS_VPI_TRACE=1: one checksum per walker and step (debugging aid)
       print '(a,2i6,*(1x,z16.16))', ' trace',iblock,istep,(transfer(sum(s%Path(:,:,:,w)),1_8),w=1,sh%NW)
    end if
    end associate
  end subroutine step_host

  ! one MC step of the device-resident sampler: the whole step of every walker in one launch (K6), queued and not waited
  ! for, so that the previous step's estimators, collected behind it, ran beside it on the context's second stream on a
  ! snapshot of the worldlines (pigs_diagonal_estimators_begin / _end: at 128 walkers per GPU the sampler leaves half of
  ! the CUs idle); then the step's events
  subroutine step_device(sh,istep)
    type(shard_state), intent(inout) :: sh
    integer, intent(in) :: istep
    integer :: w,i

    call pigs_check(pigs_sampler_step(sh%ctx,int(istep,c_int32_t)),'pigs_sampler_step')
    call collect_estimators(sh)
    if (CWorm<=0.d0) return
    ! sector of every walker after the step and what its worm did during it: the permutation-cycle bookkeeping of the
    ! reference (sample_mod.f90:530-594) is replayed from the event log
    associate (s => sh%s, perm => sh%perm, ev => sh%dev%ev)
    call pigs_check(pigs_sampler_events(sh%ctx,ev),'pigs_sampler_events')
    do w=1,sh%NW
       s%isopen(w) = ev(2,w)/=0
       if (swapping) then
          do i=1,ev(1,w)
             select case (ev(1+2*i,w))
             case (1)
                s%iworm(w) = ev(2+2*i,w)
                perm(w)%new_cycle = .true.
                call perm_sampling(perm(w),.true.,s%iworm(w))
             case (2)
                perm(w)%end_cycle = .true.
                call perm_sampling(perm(w),.false.,s%iworm(w))
             case (3)
                call perm_sampling(perm(w),.true.,s%iworm(w),ev(2+2*i,w),.true.)
             end select
          end do
       end if
    end do
    end associate
    ! the end-to-end vectors that the step's worm loops handed to the OBDM histogram (momentum = T)
    call sh%fams%nk_step(sh%ctx,sh%NW)
  end subroutine step_device

  ! the estimators of the walkers in the diagonal sector after a step (reference vpi.f90:406-473): LocalEnergy x2 (K4),
  ! ThermEnergy (K2/K3) and -- device-resident sampler, PBC -- g(r), S(k) on the device (K7) in one library call; the
  ! host-driven sampler keeps the structural estimators on its mirror.  Then the same walkers' slices into the accumulators
  ! of the estimator keys.
  subroutine queue_estimators(sh)
    type(shard_state), intent(inout) :: sh
    integer(c_int32_t) :: wl(sh%NW)
    integer :: w,nd

    nd = 0
    do w=1,sh%NW
       if (.not. sh%s%isopen(w)) then
          nd = nd+1
          sh%pend%list(nd) = w
          wl(nd) = w-1
       end if
    end do
    if (nd==0) return
    sh%pend%nd = nd
    if (device_sampler) then
       sh%pend%structure = .not. trap
       call pigs_check(pigs_diagonal_estimators_begin(sh%ctx,int(nd,c_int32_t),wl,int(Nbin,c_int32_t),rbin, &
            & int(Nk,c_int32_t),merge(1_c_int32_t,0_c_int32_t,sh%pend%structure)),'pigs_diagonal_estimators_begin')
    else
       call sampler_flush(sh%s)
       call pigs_check(pigs_diagonal_estimators(sh%ctx,int(nd,c_int32_t),wl,0_c_int32_t,0.d0,0_c_int32_t, &
            & sh%pend%en9,c_null_ptr,c_null_ptr),'pigs_diagonal_estimators')
    end if
    sh%pend%queued = .true.
    call sh%fams%queue(sh%ctx,nd,wl)
  end subroutine queue_estimators

  ! what queue_estimators left of the previous step, into the block's sums (reference vpi.f90:443-473)
  subroutine collect_estimators(sh)
    type(shard_state), intent(inout), target :: sh
    integer :: i,w
    real(8) :: E,Kin,Pot,Et,Kt

    if (.not. sh%pend%queued) return
    sh%pend%queued = .false.
    if (device_sampler) then
       if (sh%pend%structure) then
          call pigs_check(pigs_diagonal_estimators_end(sh%ctx,sh%pend%en9,c_loc(sh%pend%gr_inc),c_loc(sh%pend%sk_inc)), &
               & 'pigs_diagonal_estimators_end')
       else
          call pigs_check(pigs_diagonal_estimators_end(sh%ctx,sh%pend%en9,c_null_ptr,c_null_ptr),'pigs_diagonal_estimators_end')
       end if
    end if
    !$omp parallel do schedule(dynamic,1) private(w,E,Pot,Kin,Et,Kt) num_threads(min(sh%pend%nd,16))
    do i=1,sh%pend%nd
       w = sh%pend%list(i)
       sh%en%idiag(w) = sh%en%idiag(w)+1; sh%en%idiag_aux(w) = sh%en%idiag_aux(w)+1
       sh%en%idiag_block(w) = sh%en%idiag_block(w)+1
       E   = 0.5d0*(sh%pend%en9(1,i)+sh%pend%en9(4,i))
       Et  = sh%pend%en9(7,i); Kt = sh%pend%en9(8,i)
       Pot = sh%pend%en9(9,i)
       Kin = E-Pot
       sh%en%BE(:,w)  = sh%en%BE(:,w)+[E,Kin,Pot]
       sh%en%BT(:,w)  = sh%en%BT(:,w)+[Et,Kt,Pot]
       sh%en%BE2(:,w) = sh%en%BE2(:,w)+[E**2,Kin**2,Pot**2]
       sh%en%BT2(:,w) = sh%en%BT2(:,w)+[Et**2,Kt**2,Pot**2]
       sh%en%ngr(w) = sh%en%ngr(w)+1
       if (.not. trap) then
          if (device_sampler) then
             sh%core%gr(:,w)   = sh%core%gr(:,w)+sh%pend%gr_inc(:,i)
             sh%core%Sk(:,:,w) = sh%core%Sk(:,:,w)+sh%pend%sk_inc(:,:,i)
          else
             call pair_correlation(sh%ep,sh%s%Path(:,:,Nb,w),sh%core%gr(:,w))
             call structure_factor(sh%ep,sh%s%Path(:,:,Nb,w),sh%core%Sk(:,:,w))
          end if
       end if
    end do
    !$omp end parallel do
  end subroutine collect_estimators

  ! end of a block (reference vpi.f90:477-545): what the device counted, the families' sums, every walker's block values
  ! and lines, the block's one exchange between the shards, the walker averages
  subroutine block_end(sh,iblock)
    type(shard_state), intent(inout) :: sh
    integer, intent(in) :: iblock
    real(8) :: mE(3),mT(3)
    integer :: w,nd

    if (device_sampler) then
       call pigs_check(pigs_sampler_counters16(sh%ctx,sh%dev%acc),'pigs_sampler_counters16')
       call sh%moves%from_device(sh%dev%acc,sh%dev%acc0)
       if (CWorm>0.d0 .and. .not. trap) then
          ! the device keeps accumulating a walker's OBDM histogram until the block that normalises it
          sh%dev%reset = merge(1,0,sh%en%idiag_aux/Nstep>=1)
          call pigs_check(pigs_sampler_nrho(sh%ctx,sh%dev%nrho,sh%dev%reset),'pigs_sampler_nrho')
          sh%core%nrho = sh%dev%nrho
       end if
    end if
    call sh%fams%read(sh%ctx)
    if (.not. trap) call sh%fams%nk_read(sh%ctx,sh%en%idiag_aux/Nstep>=1)
    sh%info%iblock = iblock
    mE = 0.d0; mT = 0.d0; nd = 0
    sh%vec = 0.d0
    associate (en => sh%en)
    do w=1,sh%NW
       if (en%idiag_block(w)/=0) then
          en%BE(:,w)  = en%BE(:,w)/real(en%idiag_block(w));  en%BE2(:,w) = en%BE2(:,w)/real(en%idiag_block(w))
          en%BT(:,w)  = en%BT(:,w)/real(en%idiag_block(w));  en%BT2(:,w) = en%BT2(:,w)/real(en%idiag_block(w))
          en%diag_bl(w) = en%diag_bl(w)+1
          en%AE(:,w)  = en%AE(:,w)+en%BE(:,w);  en%AE2(:,w) = en%AE2(:,w)+en%BE(:,w)**2
          en%AT(:,w)  = en%AT(:,w)+en%BT(:,w);  en%AT2(:,w) = en%AT2(:,w)+en%BT(:,w)**2
          call sh%core%block(w,en%ngr(w),sh%vec)
          sh%info%kin = en%BE(2,w)/Np
          call sh%fams%block(w,sh%info,sh%vec)
          write (sh%ue(w),'(5g20.10e3)') real(iblock),en%BE(1,w)/Np,en%BE(2,w)/Np,en%BE(3,w)/Np
          write (sh%ut(w),'(5g20.10e3)') real(iblock),en%BT(1,w)/Np,en%BT(2,w)/Np,en%BT(3,w)/Np
          write (sh%uh(w),'(i8,6(1x,z16.16))') iblock,en%BE(1,w)/Np,en%BE(2,w)/Np,en%BE(3,w)/Np, &
               & en%BT(1,w)/Np,en%BT(2,w)/Np,en%BT(3,w)/Np
          mE = mE+en%BE(:,w)/Np; mT = mT+en%BT(:,w)/Np; nd = nd+1
       end if
       if (en%idiag_aux(w)/Nstep>=1) then
          en%obdm_bl(w) = en%obdm_bl(w)+1
          call sh%core%block_nr(w,real(en%idiag_aux(w),8),sh%vec)
          if (.not. trap) call sh%fams%nk_block(w,real(en%idiag_aux(w),8),sh%info,sh%vec)
          en%idiag_aux(w) = 0
       end if
    end do
    ! ---- the block's one exchange between the shards: all-reduce of the estimator vector
    sh%vec(1) = nd; sh%vec(2:4) = mE; sh%vec(5:7) = mT
    sh%vec(8:7+NSUMS) = sh%moves%block_sums(sum(en%idiag_block))
    end associate
    if (G>1) call pigs_check(pigs_estimators_allreduce(sh%ctx,sh%vec,int(sh%nvec,c_int32_t)),'pigs_estimators_allreduce')
    sh%tot%ndall = nint(sh%vec(1)); sh%tot%mE = sh%vec(2:4); sh%tot%mT = sh%vec(5:7); sh%tot%moves = sh%vec(8:7+NSUMS)
    ! ---- the walker average of every block value, over the walkers of all shards that counted the block
    if (sh%ish==1 .and. NWtot>1) then
       if (sh%tot%ndall>0) then
          write (sh%ueav,'(5g20.10e3)') real(iblock),sh%tot%mE/sh%tot%ndall
          write (sh%utav,'(5g20.10e3)') real(iblock),sh%tot%mT/sh%tot%ndall
       end if
       call sh%core%average(sh%vec)
       sh%info%ndall = sh%tot%ndall
       if (sh%tot%ndall>0) sh%info%kin = sh%tot%mE(2)/sh%tot%ndall
       call sh%fams%average(sh%info,sh%vec)
    end if
  end subroutine block_end

  ! checkpoint of a block (reference vpi.f90:541-545): the device-resident sampler hands its walkers' state over first
  subroutine block_checkpoint(sh)
    type(shard_state), intent(inout) :: sh
    integer(c_int32_t) :: rpos
    integer :: w
    if (device_sampler) then
       call pigs_check(pigs_path_download_all(sh%ctx,sh%s%Path),'pigs_path_download_all')
       do w=1,sh%NW
          call pigs_check(pigs_sampler_get_rng(sh%ctx,int(w-1,c_int32_t),rpos,sh%s%rng(w)%w),'pigs_sampler_get_rng')
          sh%s%rng(w)%pos = rpos
       end do
       call pigs_check(pigs_sampler_get_worm(sh%ctx,sh%dev%isopen,sh%dev%iworm,sh%s%xend),'pigs_sampler_get_worm')
       sh%s%isopen = sh%dev%isopen/=0; sh%s%iworm = sh%dev%iworm
    end if
    call write_checkpoints(sh%s,sh%w0)
  end subroutine block_checkpoint

  ! shard 1 prints the block, which took t seconds, from what the all-reduce left
  subroutine block_report(sh,iblock,t)
    type(shard_state), intent(in) :: sh
    integer, intent(in) :: iblock
    real(8), intent(in) :: t
    associate (ndall => sh%tot%ndall, m => sh%tot%moves)
    print '(a)',            ' -----------------------------------------------------------'
    print '(a,i8)',         ' BLOCK NUMBER :',iblock
    if (ndall>0) then
       print '(a,3g18.9)',  '   > <E>,<Ec>,<Ep>  =',sh%tot%mE/ndall
       print '(a,3g18.9)',  '   > <Et>,<Kt>,<Vt> =',sh%tot%mT/ndall
    end if
    print '(a,f7.2,a)',     '   > CM movements      =',100*m(SUM_ACC_CM)/max(m(SUM_TRY_CM),1.d0),' %'
    print '(a,f7.2,a)',     '   > Staging movements =',100*m(SUM_ACC_BD)/max(m(SUM_TRY_STAG),1.d0),' %'
    print '(a,f7.2,a)',     '   > Head movements    =',100*m(SUM_ACC_HEAD)/max(m(SUM_TRY_STAG),1.d0),' %'
    print '(a,f7.2,a)',     '   > Tail movements    =',100*m(SUM_ACC_TAIL)/max(m(SUM_TRY_STAG),1.d0),' %'
    print '(a,f7.2,a)',     '   > Diagonal conf.    =',100.d0*m(SUM_DIAG)/real(Nstep*NWtot),' %'
    print '(a,f7.2,a)',     '   > Open acc          =',100.d0*m(SUM_ACC_OPEN)/max(m(SUM_TRY_OPEN),1.d0),' %'
    print '(a,f7.2,a)',     '   > Close acc         =',100.d0*m(SUM_ACC_CLOSE)/max(m(SUM_TRY_CLOSE),1.d0),' %'
    print '(a,f7.2,a)',     '   > Swap acc          =',100.d0*m(SUM_ACC_SWAP)/max(m(SUM_TRY_SWAP),1.d0),' %'
    print '(a,f9.2,a,i12,a,i10,a,f9.2,a)', '   > Time per block    =',t,' s;  Delta S items so far (shard 1)',sh%s%n_eval_items, &
         & ' in',sh%s%n_eval_calls,' batches,',sh%s%t_eval,' s inside them'
    end associate
  end subroutine block_report

  ! final averages and files (reference vpi.f90:590-642), the shard's part of what the main program prints and writes,
  ! and the check of the host mirror
  subroutine shard_finish(sh)
    type(shard_state), intent(inout) :: sh
    real(8), allocatable :: chk(:,:,:,:)
    integer(c_int32_t) :: form(4)
    character(len=32)  :: suffix
    integer :: w,ip,u

    do w=1,sh%NW
       suffix = walker_suffix(sh%w0+w-1)
       close (sh%ue(w)); close (sh%ut(w)); close (sh%uh(w))
       if (swapping) then
          open (newunit=u,file='perm_vpi'//trim(suffix)//'.out')
          do ip=1,Np
             write (u,*) ip,sh%perm(w)%histogram(ip)
          end do
          close (u)
       end if
       call sh%core%write_walker(suffix,w,sh%en%diag_bl(w),sh%en%obdm_bl(w))
       call sh%fams%write_walker(suffix,w,sh%en%diag_bl(w))
    end do
    if (NWtot>1 .and. sh%ish==1) then
       close (sh%ueav); close (sh%utav)
       call sh%core%write_average()
       call sh%fams%write_average()
    end if

    do w=1,sh%NW
       AE_all(:,sh%w0+w) = sh%en%AE(:,w); AT_all(:,sh%w0+w) = sh%en%AT(:,w); diag_bl_all(sh%w0+w) = sh%en%diag_bl(w)
    end do

    ! final worldlines back from the device must equal the host mirror: the two were kept in
    ! step by commits only
    if (.not. device_sampler) call sampler_flush(sh%s)
    allocate (chk(dim,Np,0:2*Nb,sh%NW))
    call pigs_check(pigs_path_download_all(sh%ctx,chk),'pigs_path_download_all')
    if (device_sampler) sh%s%Path = chk
    if (any(chk/=sh%s%Path)) then
       write (0,*) 'pigs_vpi: device worldlines differ from the host mirror'
       stop 3
    end if
    chk_all(:,:,:,sh%w0+1:sh%w0+sh%NW) = chk

    ! the form the device-resident sampler ran its last step in (pigs_sampler_form): tests check they ran the form they meant to
    if (device_sampler .and. sh%ish==1) then
       if (sampler_form(sh%ctx,form)) print '(a,i5,a,i2,a,l2,a,l2)','  > sampler form: sweep threads',form(1), &
            & ', TranslateChain workgroups per walker',form(2),', stage machine',form(3)/=0,', shared',form(4)/=0
    end if

    call sampler_free(sh%s)
  end subroutine shard_finish

  ! what the files of walker w (global, 0-based) carry behind their name: .wNNNN, nothing in a run of one walker
  function walker_suffix(w) result(suffix)
    integer, intent(in) :: w
    character(len=32)   :: suffix
    suffix = ''
    if (NWtot>1) write (suffix,'(a,i4.4)') '.w',w
  end function walker_suffix

end program pigs_vpi
