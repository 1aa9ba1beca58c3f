!-----------------------------------------------------------------------
! pigs_families -- the per-walker accumulator families of the front end (pigs_vpi.f90), one type each.
!
! A family is what one estimator key of &gpu switches on: density_profile, fq_tau, sq_vector, gr_vector, fq_vector,
! tau_profile, fq_self, bond_order, van_hove, triplet, three_body, momentum, lattice, superfluid, clusters, percolation.  On the device it is an accumulator that takes the diagonal walkers of every step and is read and
! reset once per block; on the host it is the raw block sums of every walker, their normalisation, one block_series per
! output file and one block_count (pigs_block_stats).  Everything a family does sits in its type, in the phases the front
! end walks through:
!     check          the key's values (refused before the backend is asked), the window default, *_bind()
!     banner         its line of the run's banner
!     setup          *_init and the entry that queue calls, its grids, allocation, its claims on the block vector, the reset
!                    mask, the files with one line per block
!     queue          the family's *_accumulate for the diagonal walkers of a step: one procedure for all families
!     read           *_read at the end of a block
!     block          walker w counted the block: normalize_*, series_add per file, count_add
!     average        on the shard that writes the walker averages, after the all-reduce: count_reduced, series_average
!     write_files    every file of the family once: of walker w, or with w = 0 the walker-averaged ones
! A family_set holds one slot per family, in the order of their claims on the block vector and of every device call;
! only the slots of the keys that are on are allocated, and the set has one procedure per phase that walks them.
!
! A new family is a new extension of `family` here with these phases but queue, for which its setup names the device
! entry; a slot (and a line of set_create) in family_set; and its keys in family_keys and in the program's namelist.
! Whatever a family keeps per walker and for the walker average has the average at index 0 (block_series, the units of
! the files with one line per block), so that write_files says nothing twice.
!-----------------------------------------------------------------------
module pigs_families

  use iso_c_binding
  use pigs_capi
  use pigs_estimators
  use pigs_block_stats

  implicit none
  private
  public :: family_keys,family_run,family_info,family_set

  ! the values of the estimator keys of &gpu (the namelist itself and its defaults belong to the program)
  type family_keys
     logical :: density_profile = .false.
     logical :: fq_tau = .false.
     integer :: fq_ntau = 0, fq_window = -1
     logical :: sq_vector = .false.
     integer :: sq_nmax = 8, sq_window = 0
     logical :: gr_vector = .false.
     integer :: gr_nbin = 32, gr_window = 0
     logical :: fq_vector = .false.
     integer :: fqv_nmax = 8, fqv_ntau = 0, fqv_window = -1
     logical :: tau_profile = .false.
     integer :: tau_window = 0
     logical :: fq_self = .false.
     integer :: fqs_nmax = 8, fqs_ntau = 0, fqs_window = -1
     logical :: bond_order = .false.
     real(8) :: bo_rnb = 0.d0
     integer :: bo_nhist = 50, bo_nr = -1, bo_window = 0     ! bo_nr < 0: the run's g(r) grid
     real(8) :: half_side = 0.d0                    ! half the shortest side of a periodic box (what bo_rnb may not pass)
     logical :: van_hove = .false.
     integer :: vh_ntau = 0, vh_window = -1, vh_nself = 50
     real(8) :: vh_rself = 0.d0                     ! <= 0: the run's rcut
     logical :: triplet = .false.
     integer :: g3_nr = 10, g3_na = 20, g3_window = -1       ! g3_window < 0: slice Nb alone
     real(8) :: g3_rmax = 0.d0                      ! <= 0: the run's rcut (half the shortest side)
     logical :: three_body = .false.
     logical :: atm_nu_given = .false.              ! F: atm_nu was left out, the files hold the bare geometric sum
     real(8) :: atm_nu = 1.d0                       ! the triple-dipole coupling, in the run's units (energy length^9)
     real(8) :: atm_rc = 0.d0                       ! <= 0: half the shortest side
     integer :: atm_window = -1                     ! < 0: slice Nb alone
     logical :: momentum = .false.
     integer :: nk_nmax = 8, nk_nbin = 32
     real(8) :: cworm = 0.d0                        ! the run's CWorm and Nobdm (momentum needs the worm sector)
     integer :: nobdm = 0
     logical :: lattice = .false.
     integer :: lat_nbin = 0                        ! <= 0: the run's Nbin (nbin_run)
     real(8) :: lat_rmax = 0.d0                     ! <= 0: half the sites' nearest-neighbour distance
     integer :: lat_window = -1                     ! < 0: slice Nb alone
     logical :: lat_cm = .true.
     integer :: nbin_run = 0                        ! the run's Nbin and box (what lattice measures its sites in)
     real(8) :: box(3) = 0.d0
     integer :: lat_nsite = 0                       ! filled in by the check from config_ini.in: the sites and their
     real(8) :: lat_ann = 0.d0                      ! nearest-neighbour distance
     real(8), allocatable :: lat_sites(:,:)         ! (dim,lat_nsite)
     logical :: superfluid = .false.
     integer :: sf_ntau = 0, sf_window = -1         ! sf_window < 0: the smallest window that holds the lags
     logical :: clusters = .false.
     real(8) :: cl_rc = 0.d0                        ! <= 0: the run's rcut (half the shortest side)
     integer :: cl_window = -1                      ! < 0: 0
     logical :: percolation = .false.
     real(8) :: pc_rc = 0.d0                        ! <= 0: the run's rcut (half the shortest side)
     integer :: pc_window = -1, pc_ntau = 0         ! pc_window < 0: the smallest window that holds the lags
  end type family_keys

  ! what the families need to know of the run and of the shard
  type family_run
     integer :: Nb = 0
     real(8) :: dt = 0.d0, density = 0.d0, rcut = 0.d0
     logical :: averages = .false.                  ! this shard writes the walker-averaged files (several walkers, shard 1)
     character(len=32), allocatable :: suffix(:)    ! [NW] what the files of the shard's walkers carry behind their name
  end type family_run

  ! what only the caller knows of a block and the pressure of tau_profile needs
  type family_info
     integer :: iblock = 0
     real(8) :: kin    = 0.d0     ! block: the walker's Kin/Np of e_vpi.out; average: that of the walkers that counted the block
     integer :: ndall  = 0        ! average: how many walkers of all shards these are
  end type family_info

  type, abstract :: family
     type(family_run) :: run
     type(est_params) :: ep
     integer(c_int64_t), allocatable :: smp(:)      ! [NW] the block's samples per walker, from the device
     integer(c_int32_t), allocatable :: reset(:)    ! [NW] 1: the device zeroes the walker's sums after the copy
     type(block_count) :: cnt
     procedure(pigs_accumulate_t), pointer, nopass :: accumulate => null()     ! what queue calls, and its name in the
     character(len=24) :: entry = ''                                           ! message of a failure; both set by setup
   contains
     procedure(check_i),       deferred :: check
     procedure(banner_i),      deferred :: banner
     procedure(setup_i),       deferred :: setup
     procedure :: queue => family_queue
     procedure(read_i),        deferred :: read
     procedure(block_i),       deferred :: block
     procedure(average_i),     deferred :: average
     procedure(write_files_i), deferred :: write_files
  end type family

  abstract interface
     subroutine check_i(f,keys,dim,Nb,trap)
       import :: family,family_keys
       class(family), intent(inout)     :: f
       type(family_keys), intent(inout) :: keys
       integer, intent(in) :: dim,Nb
       logical, intent(in) :: trap
     end subroutine check_i
     subroutine banner_i(f,keys,trap)
       import :: family,family_keys
       class(family), intent(in)     :: f
       type(family_keys), intent(in) :: keys
       logical, intent(in) :: trap
     end subroutine banner_i
     subroutine setup_i(f,keys,run,ctx,ep,NW,nvec)
       import :: family,family_keys,family_run,est_params,c_ptr
       class(family), intent(inout)  :: f
       type(family_keys), intent(in) :: keys
       type(family_run), intent(in)  :: run
       type(c_ptr), intent(in)       :: ctx
       type(est_params), intent(in)  :: ep
       integer, intent(in)    :: NW
       integer, intent(inout) :: nvec
     end subroutine setup_i
     subroutine read_i(f,ctx)
       import :: family,c_ptr
       class(family), intent(inout) :: f
       type(c_ptr), intent(in)      :: ctx
     end subroutine read_i
     subroutine block_i(f,w,info,vec)
       import :: family,family_info
       class(family), intent(inout)  :: f
       integer, intent(in)           :: w
       type(family_info), intent(in) :: info
       real(8), intent(inout)        :: vec(:)
     end subroutine block_i
     subroutine average_i(f,info,vec)
       import :: family,family_info
       class(family), intent(inout)  :: f
       type(family_info), intent(in) :: info
       real(8), intent(in)           :: vec(:)
     end subroutine average_i
     ! w > 0: walker w (local index), whose files carry suffix, over the n blocks it counted; w = 0: the walker averages,
     ! suffix = '', over the n blocks that one of the walkers counted
     subroutine write_files_i(f,suffix,w,n)
       import :: family
       class(family), intent(inout) :: f
       character(len=*), intent(in) :: suffix
       integer, intent(in)          :: w,n
     end subroutine write_files_i
  end interface

  ! the stored vectors of a reciprocal grid and their |q| shells (sq_vector, fq_vector, fq_self)
  type qgrid
     integer :: nq = 0, nsh = 0
     integer(c_int32_t), allocatable :: n(:,:)      ! [dim,nq]
     integer, allocatable :: shell(:),mult(:)       ! [nq] the shell of a vector, [nsh] the vectors of a shell
     real(8), allocatable :: q(:)                   ! [nsh] |q|
  end type qgrid

  ! density profiles: the block's counts from the device and the normalised block profiles
  type, extends(family) :: density_family
     integer :: npl = 0
     integer(c_int64_t), allocatable :: pl(:,:),rad(:,:),pair(:,:)
     real(8), allocatable :: bpl(:),brad(:),bpair(:)
     type(block_series) :: sPl,sRad,sPair
   contains
     procedure :: check => density_check
     procedure :: banner => density_banner
     procedure :: setup => density_setup
     procedure :: read => density_read
     procedure :: block => density_block
     procedure :: average => density_average
     procedure :: write_files => density_write_files
  end type density_family

  ! F(q,tau) on the S(k) grid: the block's raw sums from the device and the normalised block values
  type, extends(family) :: fqt_family
     integer :: ntau = 0, window = 0
     real(8), allocatable :: raw(:,:,:,:),b(:,:,:)  ! (third index: lag l + 1)
     type(block_series) :: s
   contains
     procedure :: check => fqt_check
     procedure :: banner => fqt_banner
     procedure :: setup => fqt_setup
     procedure :: read => fqt_read_block
     procedure :: block => fqt_block
     procedure :: average => fqt_average
     procedure :: write_files => fqt_write_files
  end type fqt_family

  ! vector S(q): the block's raw sums from the device, the normalised block values per vector and per shell
  type, extends(family) :: sqv_family
     integer :: window = 0
     type(qgrid) :: g
     real(8), allocatable :: raw(:,:),b(:),sh(:)
     type(block_series) :: sVec,sSh
   contains
     procedure :: check => sqv_check
     procedure :: banner => sqv_banner
     procedure :: setup => sqv_setup
     procedure :: read => sqv_read_block
     procedure :: block => sqv_block
     procedure :: average => sqv_average
     procedure :: write_files => sqv_write_files
  end type sqv_family

  ! vector g(r): the block's counts from the device, the normalised block values on the vector grid and radially
  type, extends(family) :: grv_family
     integer :: nbin = 0, window = 0, ngb = 0
     integer(c_int64_t), allocatable :: vec(:,:),rad(:,:)
     real(8), allocatable :: bvec(:),brad(:)
     type(block_series) :: sVec,sRad
   contains
     procedure :: check => grv_check
     procedure :: banner => grv_banner
     procedure :: setup => grv_setup
     procedure :: read => grv_read_block
     procedure :: block => grv_block
     procedure :: average => grv_average
     procedure :: write_files => grv_write_files
  end type grv_family

  ! a function of (vector, lag) on the full reciprocal grid: fq_vector, and with self = T fq_self, which has the two
  ! moments of the displacement per lag beside it.  The block's raw sums from the device, the normalised block values per
  ! (vector, lag), per (shell, lag) and of the moments.  What tells the two keys apart is set by fqv_family / fqs_family.
  type, extends(family) :: lagged_family
     logical :: self = .false.
     character(len=9)  :: key = ''
     character(len=3)  :: pre = ''                  ! of the key's values (pre_nmax ..) and of the device's entry points
     character(len=25) :: what = ''                 ! in the message of a backend without it
     character(len=25) :: label = ''                ! of the banner line
     character(len=48) :: files = ''                ! at its end
     character(len=6)  :: fvec = '', fsh = ''       ! file names before _vpi
     integer :: ntau = 0, window = 0
     type(qgrid) :: g
     real(8), allocatable :: raw(:,:,:),draw(:,:,:),b(:,:),sh(:,:),bm(:,:)     ! (second index: lag l + 1)
     type(block_series) :: sVec,sSh,sMsd
   contains
     procedure :: check => lagged_check
     procedure :: banner => lagged_banner
     procedure :: setup => lagged_setup
     procedure :: read => lagged_read_block
     procedure :: block => lagged_block
     procedure :: average => lagged_average
     procedure :: write_files => lagged_write_files
  end type lagged_family

  ! imaginary-time profiles: the block's raw sums from the device (Vpair, Vext, W, D2 per slice), the normalised block
  ! profiles; the units of press_vpi*.out (periodic runs)
  type, extends(family) :: tau_family
     integer :: window = 0
     real(8), allocatable :: raw(:,:,:),b(:,:)      ! (second index: slice b + 1)
     type(block_series) :: s
     integer, allocatable :: up(:)                  ! [0:NW] the units of the file with one line per block
   contains
     procedure :: check => tau_check
     procedure :: banner => tau_banner
     procedure :: setup => tau_setup
     procedure :: read => tau_read_block
     procedure :: block => tau_block
     procedure :: average => tau_average
     procedure :: write_files => tau_write_files
  end type tau_family

  ! bond-orientational order: the block's raw sums and counts from the device, the normalised block values (the five
  ! scalars, the two distributions, G6 per radial bin); epr is ep with the radial grid of G6
  type, extends(family) :: bop_family
     integer :: nh = 0, nr = 0, window = 0
     real(8) :: rnb = 0.d0
     type(est_params) :: epr
     real(8), allocatable :: rawS(:,:),rawG(:,:),b(:),bh(:,:),bg(:)
     integer(c_int64_t), allocatable :: H(:,:,:),GN(:,:)
     type(block_series) :: sB,sH,sG
   contains
     procedure :: check => bop_check
     procedure :: banner => bop_banner
     procedure :: setup => bop_setup
     procedure :: read => bop_read_block
     procedure :: block => bop_block
     procedure :: average => bop_average
     procedure :: write_files => bop_write_files
  end type bop_family

  ! van Hove functions: the block's counts from the device and the normalised block values G_s (self grid eps) and G_d
  ! (the run's radial grid), per lag
  type, extends(family) :: vh_family
     integer :: ntau = 0, window = 0, ns = 0
     type(est_params) :: eps
     integer(c_int64_t), allocatable :: cself(:,:,:),cdist(:,:,:)
     real(8), allocatable :: bs(:,:),bd(:,:)
     type(block_series) :: sS,sD
   contains
     procedure :: check => vh_check
     procedure :: banner => vh_banner
     procedure :: setup => vh_setup
     procedure :: read => vh_read_block
     procedure :: block => vh_block
     procedure :: average => vh_average
     procedure :: write_files => vh_write_files
  end type vh_family

  ! triplet distribution: the block's counts from the device and the normalised block values g3 (packed triangle of leg
  ! bins x angle bins, on the grid epr) and P(cos theta)
  type, extends(family) :: g3_family
     integer :: na = 0, window = 0, npk = 0
     type(est_params) :: epr
     integer(c_int64_t), allocatable :: ctrip(:,:,:),cpair(:,:)
     real(8), allocatable :: b2(:),b3(:,:),ba(:)
     type(block_series) :: s3,sA
   contains
     procedure :: check => g3_check
     procedure :: banner => g3_banner
     procedure :: setup => g3_setup
     procedure :: read => g3_read_block
     procedure :: block => g3_block
     procedure :: average => g3_average
     procedure :: write_files => g3_write_files
  end type g3_family

  ! Axilrod-Teller-Muto three-body energy: the block's raw sums and triplet counts from the device per window slice, the
  ! normalised block values (V3/Np and the mean triplets per slice); the units of v3_vpi*.out
  type, extends(family) :: atm_family
     integer :: window = 0
     real(8) :: nu = 1.d0, rc = 0.d0
     real(8), allocatable :: raw(:,:),b(:,:)        ! (first index of raw, second of b: slice a - (Nb-window) + 1)
     integer(c_int64_t), allocatable :: ntrip(:,:)
     type(block_series) :: s
     integer, allocatable :: up(:)                  ! [0:NW] the units of the file with one line per block
   contains
     procedure :: check => atm_check
     procedure :: banner => atm_banner
     procedure :: setup => atm_setup
     procedure :: read => atm_read_block
     procedure :: block => atm_block
     procedure :: average => atm_average
     procedure :: write_files => atm_write_files
  end type atm_family

  ! momentum: the off-diagonal family.  Its samples are the end-to-end vectors of the open walkers, so it is queued for all
  ! walkers after a step (step / add) and not with the diagonal ones (queue does nothing); its block is the one that
  ! normalises nr_vpi.out, with zconf = idiag_aux(w) (read_nk / block_nk; read and block do nothing), and a walker's files
  ! average over the blocks it counted there (nbl).
  type, extends(family) :: nk_family
     integer :: nbin = 0, nv = 0, nobdm = 0
     type(qgrid) :: g
     real(8), allocatable :: raw(:,:),b(:),sh(:),br(:)      ! (b: index 1 is n = 0, index i + 1 the stored vector i)
     integer(c_int64_t), allocatable :: h(:,:),nopen(:),nin(:)
     integer, allocatable :: nbl(:),un(:)           ! [NW] blocks normalised, [0:NW] the units of n0_vpi*.out
     type(block_series) :: sVec,sSh,sR
   contains
     procedure :: check => nk_check
     procedure :: banner => nk_banner
     procedure :: setup => nk_setup
     procedure :: queue => nk_queue
     procedure :: read => nk_read_nothing
     procedure :: block => nk_block_nothing
     procedure :: average => nk_average
     procedure :: write_files => nk_write_files
  end type nk_family

  ! a crystal seen from its lattice: the block's raw sums from the device, the normalised block values of the three files
  ! (lind_vpi*.out per block; lindtau_vpi.out per window slice; usite_vpi.out per bin); the units of lind_vpi*.out
  type, extends(family) :: lat_family
     integer :: window = 0, nbin = 0, nsite = 0
     real(8) :: rmax = 0.d0, ann = 0.d0
     real(8), allocatable :: mom(:,:,:),bt(:,:),bu(:)
     real(8) :: bl(7)
     integer(c_int64_t), allocatable :: nass(:,:),occ(:,:,:),hr(:,:),hx(:,:,:),nlost(:),hop1(:),hopw(:)
     type(block_series) :: sL,sT,sU
     integer, allocatable :: up(:)                  ! [0:NW] the units of the file with one line per block
   contains
     procedure :: check => lat_check
     procedure :: banner => lat_banner
     procedure :: setup => lat_setup
     procedure :: read => lat_read_block
     procedure :: block => lat_block
     procedure :: average => lat_average
     procedure :: write_files => lat_write_files
  end type lat_family

  ! the superfluid fraction from the centre-of-mass diffusion along tau: the block's raw sums from the device and the
  ! normalised block values per lag (pigs_estimators normalize_sf) behind rhos_vpi.out and msdu_vpi.out
  type, extends(family) :: sf_family
     integer :: ntau = 0, window = 0
     real(8) :: lam = 0.5d0                         ! hbar^2/2m in the run's units (the spring term of ThermEnergy)
     real(8), allocatable :: c(:,:,:),d(:,:,:),b(:,:)
     integer(c_int64_t), allocatable :: nwrap(:)
     type(block_series) :: s
   contains
     procedure :: check => sf_check
     procedure :: banner => sf_banner
     procedure :: setup => sf_setup
     procedure :: read => sf_read_block
     procedure :: block => sf_block
     procedure :: average => sf_average
     procedure :: write_files => sf_write_files
  end type sf_family

  ! clusters: the block's raw sums from the device and the normalised block values per size and per block
  ! (pigs_estimators normalize_cl) behind clus_vpi.out and clusblk_vpi.out
  type, extends(family) :: cl_family
     integer :: window = 0
     real(8) :: rc = 0.d0
     integer(c_int64_t), allocatable :: nsize(:,:),nlarge(:,:),nbond(:)
     real(8), allocatable :: rg2(:,:),bs(:,:)
     real(8) :: bb(4) = 0.d0
     type(block_series) :: s,sb
     integer, allocatable :: up(:)                  ! [0:NW] the units of the file with one line per block
   contains
     procedure :: check => cl_check
     procedure :: banner => cl_banner
     procedure :: setup => cl_setup
     procedure :: read => cl_read_block
     procedure :: block => cl_block
     procedure :: average => cl_average
     procedure :: write_files => cl_write_files
  end type cl_family

  ! percolation: the block's raw sums from the device and the normalised block values per block, per size and per lag
  ! (pigs_estimators normalize_pc) behind perc_vpi.out, percsz_vpi.out and clpers_vpi.out
  type, extends(family) :: pc_family
     integer :: window = 0, ntau = 0
     real(8) :: rc = 0.d0
     integer(c_int64_t), allocatable :: nwrap(:,:),mwrap(:,:),swrap(:,:),nfin(:,:),first(:,:),second(:,:),both(:,:),norig(:,:)
     real(8), allocatable :: rg2u(:,:),bs(:,:),bp(:,:)
     real(8) :: bb(7) = 0.d0
     type(block_series) :: ss,sp,sb
     integer, allocatable :: up(:)                  ! [0:NW] the units of the file with one line per block
   contains
     procedure :: check => pc_check
     procedure :: banner => pc_banner
     procedure :: setup => pc_setup
     procedure :: read => pc_read_block
     procedure :: block => pc_block
     procedure :: average => pc_average
     procedure :: write_files => pc_write_files
  end type pc_family

  integer, parameter :: NFAM = 16
  ! the order in which the keys are checked and in which the banner names them (numbers of the slots below)
  integer, parameter :: CHECK_ORDER(NFAM)  = [1,2,3,4,5,7,6,8,9,10,11,12,13,14,15,16]
  integer, parameter :: BANNER_ORDER(NFAM) = [1,2,6,3,4,5,7,8,9,10,11,12,13,14,15,16]

  type family_slot
     class(family), allocatable :: f
  end type family_slot

  ! slots: 1 density_profile, 2 fq_tau, 3 sq_vector, 4 gr_vector, 5 fq_vector, 6 tau_profile, 7 fq_self, 8 bond_order,
  ! 9 van_hove, 10 triplet, 11 three_body, 12 momentum, 13 lattice, 14 superfluid, 15 clusters,
  ! 16 percolation
  type family_set
     type(family_slot) :: slot(NFAM)
   contains
     procedure :: create => set_create
     procedure :: check => set_check
     procedure :: banner => set_banner
     procedure :: setup => set_setup
     procedure :: queue => set_queue
     procedure :: read => set_read
     procedure :: block => set_block
     procedure :: average => set_average
     procedure :: write_walker => set_write_walker
     procedure :: write_average => set_write_average
     procedure :: nk_step => set_nk_step
     procedure :: nk_add => set_nk_add
     procedure :: nk_read => set_nk_read
     procedure :: nk_block => set_nk_block
  end type family_set

contains

  !---------------------------------------------------------------------
  ! the set: one procedure per phase

  ! the slots of the keys that are on
  subroutine set_create(fs,keys)
    class(family_set), intent(inout) :: fs
    type(family_keys), intent(in)    :: keys
    if (keys%density_profile) allocate (density_family :: fs%slot(1)%f)
    if (keys%fq_tau)          allocate (fqt_family :: fs%slot(2)%f)
    if (keys%sq_vector)       allocate (sqv_family :: fs%slot(3)%f)
    if (keys%gr_vector)       allocate (grv_family :: fs%slot(4)%f)
    if (keys%fq_vector)       allocate (fs%slot(5)%f,source=fqv_family())
    if (keys%tau_profile)     allocate (tau_family :: fs%slot(6)%f)
    if (keys%fq_self)         allocate (fs%slot(7)%f,source=fqs_family())
    if (keys%bond_order)      allocate (bop_family :: fs%slot(8)%f)
    if (keys%van_hove)        allocate (vh_family :: fs%slot(9)%f)
    if (keys%triplet)         allocate (g3_family :: fs%slot(10)%f)
    if (keys%three_body)      allocate (atm_family :: fs%slot(11)%f)
    if (keys%momentum)        allocate (nk_family :: fs%slot(12)%f)
    if (keys%lattice)         allocate (lat_family :: fs%slot(13)%f)
    if (keys%superfluid)      allocate (sf_family :: fs%slot(14)%f)
    if (keys%clusters)        allocate (cl_family :: fs%slot(15)%f)
    if (keys%percolation)     allocate (pc_family :: fs%slot(16)%f)
  end subroutine set_create

  ! momentum, device-resident sampler: the samples of the step just queued, of all NW walkers
  subroutine set_nk_step(fs,ctx,NW)
    class(family_set), intent(inout) :: fs
    type(c_ptr), intent(in) :: ctx
    integer, intent(in)     :: NW
    integer :: w
    if (.not. allocated(fs%slot(12)%f)) return
    call pigs_check(nk_accumulate(ctx,int(NW,c_int32_t),[(int(w-1,c_int32_t),w=1,NW)]),'pigs_nk_accumulate')
  end subroutine set_nk_step

  ! momentum, host-driven sampler: xend(dim,2,NW) of the walkers with act, where their OBDM histogram is taken
  subroutine set_nk_add(fs,ctx,NW,act,xend)
    class(family_set), intent(inout) :: fs
    type(c_ptr), intent(in) :: ctx
    integer, intent(in)     :: NW
    logical, intent(in)     :: act(NW)
    real(8), intent(in)     :: xend(:,:,:)
    integer(c_int32_t) :: wl(NW),ns(NW)
    real(8) :: x(size(xend,1),2,NW)
    integer :: w,n
    if (.not. allocated(fs%slot(12)%f)) return
    n = 0
    do w=1,NW
       if (.not. act(w)) cycle
       n = n+1
       wl(n) = w-1; ns(n) = 1; x(:,:,n) = xend(:,:,w)
    end do
    if (n>0) call pigs_check(nk_add(ctx,int(n,c_int32_t),wl,ns,x),'pigs_nk_add')
  end subroutine set_nk_add

  ! momentum, end of a block: the sums of every walker; those of the walkers with norm are zeroed on the device (the others
  ! go on accumulating until the block that normalises them, like the OBDM histogram)
  subroutine set_nk_read(fs,ctx,norm)
    class(family_set), intent(inout) :: fs
    type(c_ptr), intent(in) :: ctx
    logical, intent(in)     :: norm(:)
    if (.not. allocated(fs%slot(12)%f)) return
    select type (f => fs%slot(12)%f)
    type is (nk_family)
       f%reset = merge(1_c_int32_t,0_c_int32_t,norm)
       call pigs_check(nk_read(ctx,f%raw,f%h,f%nopen,f%nin,f%reset),'pigs_nk_read')
    end select
  end subroutine set_nk_read

  ! momentum: walker w normalises the block, with zconf diagonal configurations
  subroutine set_nk_block(fs,w,zconf,info,vec)
    class(family_set), intent(inout) :: fs
    integer, intent(in)           :: w
    real(8), intent(in)           :: zconf
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    if (.not. allocated(fs%slot(12)%f)) return
    select type (f => fs%slot(12)%f)
    type is (nk_family)
       call normalize_nk(f%ep%CWorm,zconf,f%nobdm,f%g%nq,f%raw(:,w),int(f%nopen(w),8),f%b)
       call sqv_shell_means(f%g%nq,f%g%shell,f%g%nsh,f%g%mult,f%b(2:),f%sh)
       call normalize_nrvec(f%ep,f%ep%CWorm,zconf,f%nobdm,f%run%density,f%nbin,f%nv,int(f%h(:,w),8),f%br)
       call series_add(f%sVec,w,f%b,vec)
       call series_add(f%sSh,w,f%sh,vec)
       call series_add(f%sR,w,f%br,vec)
       call count_add(f%cnt,vec)
       f%nbl(w) = f%nbl(w)+1
       call write_n0_block(f%un(w),info%iblock,f%ep%Np,f%b(1))
    end select
  end subroutine set_nk_block

  ! refuses what the keys cannot have (exit status 2) and fills in the windows that were left out
  subroutine set_check(fs,keys,dim,Nb,trap)
    class(family_set), intent(inout) :: fs
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(CHECK_ORDER(i))%f)) call fs%slot(CHECK_ORDER(i))%f%check(keys,dim,Nb,trap)
    end do
  end subroutine set_check

  subroutine set_banner(fs,keys,trap)
    class(family_set), intent(in) :: fs
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(BANNER_ORDER(i))%f)) call fs%slot(BANNER_ORDER(i))%f%banner(keys,trap)
    end do
  end subroutine set_banner

  ! nvec: the layout counter of the block vector, which every family moves past its claims
  subroutine set_setup(fs,keys,run,ctx,ep,NW,nvec)
    class(family_set), intent(inout) :: fs
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(i)%f)) call fs%slot(i)%f%setup(keys,run,ctx,ep,NW,nvec)
    end do
  end subroutine set_setup

  ! the slices of the diagonal walkers wl(1:nd) (0-based) of a step into every family's accumulators: queued on the
  ! context's stream behind the snapshot of the overlapped estimators (device-resident sampler) / the flushed commits
  ! (host-driven), before the next step.  Diagonal-sector walkers only: an open worm cuts the worldline at Nb.
  subroutine set_queue(fs,ctx,nd,wl)
    class(family_set), intent(inout) :: fs
    type(c_ptr), intent(in) :: ctx
    integer, intent(in)     :: nd
    integer(c_int32_t), intent(in) :: wl(:)
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(i)%f)) call fs%slot(i)%f%queue(ctx,nd,wl)
    end do
  end subroutine set_queue

  subroutine set_read(fs,ctx)
    class(family_set), intent(inout) :: fs
    type(c_ptr), intent(in) :: ctx
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(i)%f)) call fs%slot(i)%f%read(ctx)
    end do
  end subroutine set_read

  subroutine set_block(fs,w,info,vec)
    class(family_set), intent(inout) :: fs
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(i)%f)) call fs%slot(i)%f%block(w,info,vec)
    end do
  end subroutine set_block

  subroutine set_average(fs,info,vec)
    class(family_set), intent(inout) :: fs
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(i)%f)) call fs%slot(i)%f%average(info,vec)
    end do
  end subroutine set_average

  ! the files of walker w (local index), which counted nblocks blocks
  subroutine set_write_walker(fs,suffix,w,nblocks)
    class(family_set), intent(inout) :: fs
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,nblocks
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(i)%f)) call fs%slot(i)%f%write_files(suffix,w,nblocks)
    end do
  end subroutine set_write_walker

  ! the walker-averaged files, from the reduced block vectors: every family over the blocks that one of its walkers counted
  subroutine set_write_average(fs)
    class(family_set), intent(inout) :: fs
    integer :: i
    do i=1,NFAM
       if (allocated(fs%slot(i)%f)) call fs%slot(i)%f%write_files('',0,fs%slot(i)%f%cnt%nav)
    end do
  end subroutine set_write_average

  !---------------------------------------------------------------------
  ! shared by the families

  ! what every setup starts with; every walker's sums are zeroed after every read
  subroutine family_begin(f,run,ep,NW)
    class(family), intent(inout) :: f
    type(family_run), intent(in) :: run
    type(est_params), intent(in) :: ep
    integer, intent(in) :: NW
    f%run = run
    f%ep  = ep
    allocate (f%smp(NW),f%reset(NW))
    f%reset = 1
  end subroutine family_begin

  ! what every family but momentum queues for the diagonal walkers of a step
  subroutine family_queue(f,ctx,nd,wl)
    class(family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    integer, intent(in)     :: nd
    integer(c_int32_t), intent(in) :: wl(:)
    call pigs_check(f%accumulate(ctx,int(nd,c_int32_t),wl),trim(f%entry))
  end subroutine family_queue

  subroutine needs_periodic(key,why)
    character(len=*), intent(in) :: key,why
    write (0,'(a)') ' pigs_vpi: '//key//' = T needs a periodic system (trap = F): '//why
    stop 2
  end subroutine needs_periodic

  ! the entry points are resolved at run time, only for the keys that are on, so that the front end still links against
  ! backends without them
  subroutine no_backend(key,entries,what_runs)
    character(len=*), intent(in) :: key,entries,what_runs
    write (0,'(a)') ' pigs_vpi: '//key//' = T: this backend does not export '//entries//' ('//what_runs// &
         & ' on libpigs_hip.so only)'
    stop 2
  end subroutine no_backend

  ! a window of slices Nb-window..Nb+window on the path
  subroutine check_window(key,pre,window,Nb)
    character(len=*), intent(in) :: key,pre
    integer, intent(in) :: window,Nb
    if (window<0 .or. window>Nb) then
       write (0,'(a,i0,a,i0)') ' pigs_vpi: '//key//' = T: '//pre//'_window = ',window,' must lie in 0 .. Nb = ',Nb
       stop 2
    end if
  end subroutine check_window

  ! pre_nmax within what the device stores
  subroutine check_vectors(key,pre,nmax,dim)
    character(len=*), intent(in) :: key,pre
    integer, intent(in) :: nmax,dim
    if (nmax<1 .or. nmax>merge(16,64,dim==3)) then
       write (0,'(a,i0,a,i0,a,i0,a)') ' pigs_vpi: '//key//' = T: '//pre//'_nmax = ',nmax,' must lie in 1 .. ',merge(16,64,dim==3), &
            & ' (dim = ',dim,')'
       stop 2
    end if
  end subroutine check_vectors

  ! the lags 0..pre_ntau within the window Nb-pre_window..Nb+pre_window (left out: the smallest window that holds them),
  ! the window on the path
  subroutine check_lags(key,pre,ntau,window,Nb)
    character(len=*), intent(in) :: key,pre
    integer, intent(in)    :: ntau,Nb
    integer, intent(inout) :: window
    if (window<0) window = (max(ntau,0)+1)/2                   ! ceiling(ntau/2)
    if (ntau<0 .or. ntau>2*window) then
       write (0,'(a,i0,a,i0,a)') ' pigs_vpi: '//key//' = T: '//pre//'_ntau = ',ntau,' must lie in 0 .. 2*'//pre//'_window = ',2*window, &
            & ' (lags between the slices Nb-'//pre//'_window .. Nb+'//pre//'_window)'
       stop 2
    end if
    if (window>Nb) then
       write (0,'(a,i0,a,i0)') ' pigs_vpi: '//key//' = T: '//pre//'_window = ',window,' must not exceed Nb = ',Nb
       stop 2
    end if
  end subroutine check_lags

  ! the keys of fq_vector and fq_self (pre = fqv, fqs)
  subroutine check_vectors_and_lags(key,pre,dim,Nb,nmax,ntau,window)
    character(len=*), intent(in) :: key,pre
    integer, intent(in)    :: dim,Nb,nmax,ntau
    integer, intent(inout) :: window
    call check_vectors(key,pre,nmax,dim)
    call check_lags(key,pre,ntau,window,Nb)
  end subroutine check_vectors_and_lags

  ! the vectors the device stored at its *_init and their |q| shells; entries: the family's pigs_<entries>_count / _vectors
  subroutine qgrid_fill(g,ctx,ep,count,vectors,entries)
    type(qgrid), intent(out)     :: g
    type(c_ptr), intent(in)      :: ctx
    type(est_params), intent(in) :: ep
    procedure(pigs_sqv_count_t), pointer, intent(in)   :: count
    procedure(pigs_sqv_vectors_t), pointer, intent(in) :: vectors
    character(len=*), intent(in) :: entries
    integer(c_int64_t) :: nq
    call pigs_check(count(ctx,nq),entries//'_count')
    g%nq = int(nq)
    allocate (g%n(ep%dim,g%nq),g%shell(g%nq))
    call pigs_check(vectors(ctx,g%n),entries//'_vectors')
    call sqv_shells(ep,g%nq,g%n,g%shell,g%nsh,g%q,g%mult)
  end subroutine qgrid_fill

  ! the |q|-shell means of every lag of F(Nq,0:Ntau)
  subroutine shell_means_lags(Nq,shell,nsh,mult,Ntau,F,Fsh)
    integer, intent(in)  :: Nq,nsh,shell(Nq),mult(nsh),Ntau
    real(8), intent(in)  :: F(Nq,0:Ntau)
    real(8), intent(out) :: Fsh(nsh,0:Ntau)
    integer :: l
    do l=0,Ntau
       call sqv_shell_means(Nq,shell,nsh,mult,F(:,l),Fsh(:,l))
    end do
  end subroutine shell_means_lags

  ! W/Np of the profiles T averaged over the slices Nb-window..Nb+window
  function virial_window(Nb,window,T) result(wwin)
    integer, intent(in) :: Nb,window
    real(8), intent(in) :: T(4,2*Nb+1)
    real(8) :: wwin
    wwin = sum(T(3,Nb+1-window:Nb+1+window))/real(2*window+1,8)
  end function virial_window

  ! first line of press_vpi*.out
  subroutine press_header(u,window)
    integer, intent(in) :: u,window
    write (u,'(a,i0,a,i0,a)') '# block, W/Np = <sum r dv/dr>/Np over the slices Nb-',window,'..Nb+',window, &
         & ' (W stops at rcut: pairs beyond it are not counted, no tail correction), Kin/Np as e_vpi.out, '// &
         & 'P = density/dim (2 Kin/Np - W/Np)'
  end subroutine press_header

  !---------------------------------------------------------------------
  ! density_profile: the profiles of a trapped system (the reference's dead DensityProfile, vpi.f90:471), slice Nb --
  ! dens_vpi.out, rho_vpi.out, pr_vpi.out; grid half-width rcut/2

  subroutine density_check(f,keys,dim,Nb,trap)
    class(density_family), intent(inout) :: f
    type(family_keys), intent(inout)     :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (.not. trap) then
       write (0,'(a)') ' pigs_vpi: density_profile = T needs a trapped system (trap = T): periodic runs write g(r) instead'
       stop 2
    end if
    if (.not. density_bind()) call no_backend('density_profile','pigs_density_init / _accumulate / _read','the density profiles run')
  end subroutine density_check

  subroutine density_banner(f,keys,trap)
    class(density_family), intent(in) :: f
    type(family_keys), intent(in)     :: keys
    logical, intent(in) :: trap
    print '(a)',    '  > Density profiles    : on (slice Nb: dens_vpi.out, rho_vpi.out, pr_vpi.out)'
  end subroutine density_banner

  subroutine density_setup(f,keys,run,ctx,ep,NW,nvec)
    class(density_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    call family_begin(f,run,ep,NW)
    f%npl = ep%Nbin**min(ep%dim,2)
    allocate (f%pl(f%npl,NW),f%rad(ep%Nbin,NW),f%pair(ep%Nbin,NW),f%bpl(f%npl),f%brad(ep%Nbin),f%bpair(ep%Nbin))
    call series_create(f%sPl,f%npl,NW,nvec)
    call series_create(f%sRad,ep%Nbin,NW,nvec)
    call series_create(f%sPair,ep%Nbin,NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(dens_init(ctx,int(ep%Nbin,c_int32_t),run%rcut/2.d0),'pigs_density_init')
    f%accumulate => dens_accumulate; f%entry = 'pigs_density_accumulate'
  end subroutine density_setup

  subroutine density_read(f,ctx)
    class(density_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(dens_read(ctx,f%pl,f%rad,f%pair,f%smp,f%reset),'pigs_density_read')
  end subroutine density_read

  subroutine density_block(f,w,info,vec)
    class(density_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_density(f%ep%dim,f%ep%Np,f%ep%Nbin,f%run%rcut/2.d0,int(f%smp(w),8),f%pl(:,w),f%rad(:,w),f%pair(:,w), &
         & f%bpl,f%brad,f%bpair)
    call series_add(f%sPl,w,f%bpl,vec)
    call series_add(f%sRad,w,f%brad,vec)
    call series_add(f%sPair,w,f%bpair,vec)
    call count_add(f%cnt,vec)
  end subroutine density_block

  subroutine density_average(f,info,vec)
    class(density_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%sPl,vec,nall)
       call series_average(f%sRad,vec,nall)
       call series_average(f%sPair,vec,nall)
    end if
  end subroutine density_average

  subroutine density_write_files(f,suffix,w,n)
    class(density_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_density('dens_vpi'//trim(suffix)//'.out',f%ep%dim,f%ep%Nbin,f%run%rcut/2.d0,n,f%sPl%sum(:,w),f%sPl%sq(:,w))
    call write_profile('rho_vpi'//trim(suffix)//'.out',f%ep%Nbin,f%run%rcut/2.d0,n,f%sRad%sum(:,w),f%sRad%sq(:,w))
    call write_profile('pr_vpi'//trim(suffix)//'.out',f%ep%Nbin,f%run%rcut/2.d0,n,f%sPair%sum(:,w),f%sPair%sq(:,w))
  end subroutine density_write_files

  !---------------------------------------------------------------------
  ! fq_tau: imaginary-time density correlations of a periodic system on the S(k) grid, lags 0..fq_ntau between the slices
  ! Nb-fq_window..Nb+fq_window -- fqt_vpi.out

  subroutine fqt_check(f,keys,dim,Nb,trap)
    class(fqt_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('fq_tau','its q grid is that of the box')
    call check_lags('fq_tau','fq',keys%fq_ntau,keys%fq_window,Nb)
    if (.not. fqt_bind()) call no_backend('fq_tau','pigs_fqt_init / _accumulate / _read','F(q,tau) runs')
  end subroutine fqt_check

  subroutine fqt_banner(f,keys,trap)
    class(fqt_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,i0,a,i0,a,i0,a)', '  > F(q,tau)            : on (lags 0..',keys%fq_ntau,', slices Nb-',keys%fq_window,'..Nb+',keys%fq_window, &
         & ': fqt_vpi.out)'
  end subroutine fqt_banner

  subroutine fqt_setup(f,keys,run,ctx,ep,NW,nvec)
    class(fqt_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    call family_begin(f,run,ep,NW)
    f%ntau = keys%fq_ntau; f%window = keys%fq_window
    allocate (f%raw(ep%dim,ep%Nk,f%ntau+1,NW),f%b(ep%dim,ep%Nk,f%ntau+1))
    call series_create(f%s,ep%dim*ep%Nk*(f%ntau+1),NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(fqt_init(ctx,int(ep%Nk,c_int32_t),int(f%ntau,c_int32_t),int(f%window,c_int32_t)),'pigs_fqt_init')
    f%accumulate => fqt_accumulate; f%entry = 'pigs_fqt_accumulate'
  end subroutine fqt_setup

  subroutine fqt_read_block(f,ctx)
    class(fqt_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(fqt_read(ctx,f%raw,f%smp,f%reset),'pigs_fqt_read')
  end subroutine fqt_read_block

  subroutine fqt_block(f,w,info,vec)
    class(fqt_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_fqt(f%ep,f%ntau,f%window,int(f%smp(w),8),f%raw(:,:,:,w),f%b)
    call series_add(f%s,w,f%b,vec)
    call count_add(f%cnt,vec)
  end subroutine fqt_block

  subroutine fqt_average(f,info,vec)
    class(fqt_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) call series_average(f%s,vec,nall)
  end subroutine fqt_average

  subroutine fqt_write_files(f,suffix,w,n)
    class(fqt_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_fqt('fqt_vpi'//trim(suffix)//'.out',f%ep,f%ntau,f%window,f%run%dt,n,f%s%sum(:,w),f%s%sq(:,w))
  end subroutine fqt_write_files

  !---------------------------------------------------------------------
  ! sq_vector: the structure factor on the full reciprocal grid of a periodic system, averaged over the slices
  ! Nb-sq_window..Nb+sq_window -- sqvec_vpi.out, one line per vector, and sq_vpi.out, one line per |q| shell

  subroutine sqv_check(f,keys,dim,Nb,trap)
    class(sqv_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('sq_vector','its q grid is that of the box')
    call check_vectors('sq_vector','sq',keys%sq_nmax,dim)
    call check_window('sq_vector','sq',keys%sq_window,Nb)
    if (.not. sqv_bind()) call no_backend('sq_vector','pigs_sqv_init / _count / _vectors / _accumulate / _read', &
         & 'the vector S(q) runs')
  end subroutine sqv_check

  subroutine sqv_banner(f,keys,trap)
    class(sqv_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,i0,a,i0,a,i0,a)', '  > Vector S(q)         : on (|n_k| <= ',keys%sq_nmax,', slices Nb-',keys%sq_window,'..Nb+',keys%sq_window, &
         & ': sqvec_vpi.out, sq_vpi.out)'
  end subroutine sqv_banner

  subroutine sqv_setup(f,keys,run,ctx,ep,NW,nvec)
    class(sqv_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    call family_begin(f,run,ep,NW)
    f%window = keys%sq_window
    call pigs_check(sqv_init(ctx,int(keys%sq_nmax,c_int32_t),int(f%window,c_int32_t)),'pigs_sqv_init')
    f%accumulate => sqv_accumulate; f%entry = 'pigs_sqv_accumulate'
    call qgrid_fill(f%g,ctx,ep,sqv_count,sqv_vectors,'pigs_sqv')
    allocate (f%raw(f%g%nq,NW),f%b(f%g%nq),f%sh(f%g%nsh))
    call series_create(f%sVec,f%g%nq,NW,nvec)
    call series_create(f%sSh,f%g%nsh,NW)
    call count_create(f%cnt,nvec)
  end subroutine sqv_setup

  subroutine sqv_read_block(f,ctx)
    class(sqv_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(sqv_read(ctx,f%raw,f%smp,f%reset),'pigs_sqv_read')
  end subroutine sqv_read_block

  subroutine sqv_block(f,w,info,vec)
    class(sqv_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_sqv(f%ep%Np,f%window,int(f%smp(w),8),f%g%nq,f%raw(:,w),f%b)
    call sqv_shell_means(f%g%nq,f%g%shell,f%g%nsh,f%g%mult,f%b,f%sh)
    call series_add(f%sVec,w,f%b,vec)
    call series_add(f%sSh,w,f%sh,vec)
    call count_add(f%cnt,vec)
  end subroutine sqv_block

  ! (the shell means are those of the averaged vectors)
  subroutine sqv_average(f,info,vec)
    class(sqv_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%sVec,vec,nall)
       call sqv_shell_means(f%g%nq,f%g%shell,f%g%nsh,f%g%mult,f%sVec%mean,f%sh)
       call series_add_mean(f%sSh,f%sh)
    end if
  end subroutine sqv_average

  subroutine sqv_write_files(f,suffix,w,n)
    class(sqv_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_sqvec('sqvec_vpi'//trim(suffix)//'.out',f%ep,f%g%nq,f%g%n,n,f%sVec%sum(:,w),f%sVec%sq(:,w))
    call write_sqshell('sq_vpi'//trim(suffix)//'.out',f%g%nsh,f%g%q,f%g%mult,n,f%sSh%sum(:,w),f%sSh%sq(:,w))
  end subroutine sqv_write_files

  !---------------------------------------------------------------------
  ! gr_vector: the pair distribution on the Cartesian grid of the minimum-image cell of a periodic system, gr_nbin bins
  ! per axis, and radially on the run's own Nbin/rbin grid, over the slices Nb-gr_window..Nb+gr_window -- grvec_vpi.out,
  ! one line per bin, and grw_vpi.out in gr_vpi.out's format

  subroutine grv_check(f,keys,dim,Nb,trap)
    class(grv_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('gr_vector','its grid is the minimum-image cell of the box')
    if (keys%gr_nbin<1 .or. keys%gr_nbin>merge(128,merge(1024,4096,dim==2),dim==3)) then
       write (0,'(a,i0,a,i0,a,i0,a)') ' pigs_vpi: gr_vector = T: gr_nbin = ',keys%gr_nbin,' must lie in 1 .. ', &
            & merge(128,merge(1024,4096,dim==2),dim==3),' (dim = ',dim,')'
       stop 2
    end if
    call check_window('gr_vector','gr',keys%gr_window,Nb)
    if (.not. grv_bind()) call no_backend('gr_vector','pigs_grv_init / _accumulate / _read','the vector g(r) runs')
  end subroutine grv_check

  subroutine grv_banner(f,keys,trap)
    class(grv_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,i0,a,i0,a,i0,a)', '  > Vector g(r)         : on (',keys%gr_nbin,' bins per axis, slices Nb-',keys%gr_window,'..Nb+',keys%gr_window, &
         & ': grvec_vpi.out, grw_vpi.out)'
  end subroutine grv_banner

  subroutine grv_setup(f,keys,run,ctx,ep,NW,nvec)
    class(grv_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    call family_begin(f,run,ep,NW)
    f%nbin = keys%gr_nbin; f%window = keys%gr_window
    call pigs_check(grv_init(ctx,int(f%nbin,c_int32_t),int(ep%Nbin,c_int32_t),real(ep%rbin,c_double),int(f%window,c_int32_t)), &
         & 'pigs_grv_init')
    f%accumulate => grv_accumulate; f%entry = 'pigs_grv_accumulate'
    f%ngb = f%nbin**ep%dim
    allocate (f%vec(f%ngb,NW),f%rad(ep%Nbin,NW),f%bvec(f%ngb),f%brad(ep%Nbin))
    call series_create(f%sVec,f%ngb,NW,nvec)
    call series_create(f%sRad,ep%Nbin,NW,nvec)
    call count_create(f%cnt,nvec)
  end subroutine grv_setup

  subroutine grv_read_block(f,ctx)
    class(grv_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(grv_read(ctx,f%vec,f%rad,f%smp,f%reset),'pigs_grv_read')
  end subroutine grv_read_block

  subroutine grv_block(f,w,info,vec)
    class(grv_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_grv(f%ep,f%run%density,f%window,int(f%smp(w),8),f%nbin,f%ngb,f%vec(:,w),f%rad(:,w),f%bvec,f%brad)
    call series_add(f%sVec,w,f%bvec,vec)
    call series_add(f%sRad,w,f%brad,vec)
    call count_add(f%cnt,vec)
  end subroutine grv_block

  subroutine grv_average(f,info,vec)
    class(grv_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%sVec,vec,nall)
       call series_average(f%sRad,vec,nall)
    end if
  end subroutine grv_average

  subroutine grv_write_files(f,suffix,w,n)
    class(grv_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_grvec('grvec_vpi'//trim(suffix)//'.out',f%ep,f%nbin,f%ngb,n,f%sVec%sum(:,w),f%sVec%sq(:,w))
    call write_radial('grw_vpi'//trim(suffix)//'.out',f%ep,n,f%sRad%sum(:,w),f%sRad%sq(:,w))
  end subroutine grv_write_files

  !---------------------------------------------------------------------
  ! fq_vector: F(q,tau_l) on the full reciprocal grid of a periodic system, the vectors of sq_vector with |n_k| <=
  ! fqv_nmax, lags 0..fqv_ntau between the slices Nb-fqv_window..Nb+fqv_window -- fqvec_vpi.out, one line per (lag,
  ! vector), and fqsh_vpi.out, one line per (lag, |q| shell).
  ! fq_self: the self (incoherent) part F_s(q,tau_l) in the same form -- fqself_vpi.out, fqssh_vpi.out -- and the
  ! imaginary-time mean-square displacement with its fourth moment -- msd_vpi.out, one line per lag.

  function fqv_family() result(f)
    type(lagged_family) :: f
    f%self = .false.; f%key = 'fq_vector'; f%pre = 'fqv'; f%what = 'the vector F(q,tau)'
    f%label = '  > Vector F(q,tau)   :'; f%files = 'fqvec_vpi.out, fqsh_vpi.out'; f%fvec = 'fqvec'; f%fsh = 'fqsh'
  end function fqv_family

  function fqs_family() result(f)
    type(lagged_family) :: f
    f%self = .true.; f%key = 'fq_self'; f%pre = 'fqs'; f%what = 'the self part of F(q,tau)'
    f%label = '  > Self F_s(q,tau)     :'; f%files = 'fqself_vpi.out, fqssh_vpi.out, msd_vpi.out'; f%fvec = 'fqself'; f%fsh = 'fqssh'
  end function fqs_family

  subroutine lagged_check(f,keys,dim,Nb,trap)
    class(lagged_family), intent(inout) :: f
    type(family_keys), intent(inout)    :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    logical :: bound
    if (trap) call needs_periodic(trim(f%key),'its q grid is that of the box')
    if (f%self) then
       call check_vectors_and_lags(trim(f%key),f%pre,dim,Nb,keys%fqs_nmax,keys%fqs_ntau,keys%fqs_window)
       bound = fqs_bind()
    else
       call check_vectors_and_lags(trim(f%key),f%pre,dim,Nb,keys%fqv_nmax,keys%fqv_ntau,keys%fqv_window)
       bound = fqv_bind()
    end if
    if (.not. bound) call no_backend(trim(f%key),'pigs_'//f%pre//'_init / _count / _vectors / _accumulate / _read', &
         & trim(f%what)//' runs')
  end subroutine lagged_check

  ! the key's values: fqs_* with self, fqv_* without
  subroutine lagged_keys(f,keys,nmax,ntau,window)
    class(lagged_family), intent(in) :: f
    type(family_keys), intent(in)    :: keys
    integer, intent(out) :: nmax,ntau,window
    if (f%self) then
       nmax = keys%fqs_nmax; ntau = keys%fqs_ntau; window = keys%fqs_window
    else
       nmax = keys%fqv_nmax; ntau = keys%fqv_ntau; window = keys%fqv_window
    end if
  end subroutine lagged_keys

  subroutine lagged_banner(f,keys,trap)
    class(lagged_family), intent(in) :: f
    type(family_keys), intent(in)    :: keys
    logical, intent(in) :: trap
    integer :: nmax,ntau,window
    call lagged_keys(f,keys,nmax,ntau,window)
    print '(a,i0,a,i0,a,i0,a,i0,a)', trim(f%label)//' on (|n_k| <= ',nmax,', lags 0..',ntau,', slices Nb-',window, &
         & '..Nb+',window,': '//trim(f%files)//')'
  end subroutine lagged_banner

  subroutine lagged_setup(f,keys,run,ctx,ep,NW,nvec)
    class(lagged_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    integer :: nmax
    call family_begin(f,run,ep,NW)
    call lagged_keys(f,keys,nmax,f%ntau,f%window)
    if (f%self) then
       call pigs_check(fqs_init(ctx,int(nmax,c_int32_t),int(f%ntau,c_int32_t),int(f%window,c_int32_t)),'pigs_fqs_init')
       f%accumulate => fqs_accumulate; f%entry = 'pigs_fqs_accumulate'
       call qgrid_fill(f%g,ctx,ep,fqs_count,fqs_vectors,'pigs_fqs')
       allocate (f%draw(2,f%ntau+1,NW),f%bm(2,f%ntau+1))
    else
       call pigs_check(fqv_init(ctx,int(nmax,c_int32_t),int(f%ntau,c_int32_t),int(f%window,c_int32_t)),'pigs_fqv_init')
       f%accumulate => fqv_accumulate; f%entry = 'pigs_fqv_accumulate'
       call qgrid_fill(f%g,ctx,ep,fqv_count,fqv_vectors,'pigs_fqv')
    end if
    allocate (f%raw(f%g%nq,f%ntau+1,NW),f%b(f%g%nq,f%ntau+1),f%sh(f%g%nsh,f%ntau+1))
    call series_create(f%sVec,f%g%nq*(f%ntau+1),NW,nvec)
    if (f%self) call series_create(f%sMsd,2*(f%ntau+1),NW,nvec)
    call series_create(f%sSh,f%g%nsh*(f%ntau+1),NW)
    call count_create(f%cnt,nvec)
  end subroutine lagged_setup

  subroutine lagged_read_block(f,ctx)
    class(lagged_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    if (f%self) then
       call pigs_check(fqs_read(ctx,f%raw,f%draw,f%smp,f%reset),'pigs_fqs_read')
    else
       call pigs_check(fqv_read(ctx,f%raw,f%smp,f%reset),'pigs_fqv_read')
    end if
  end subroutine lagged_read_block

  subroutine lagged_block(f,w,info,vec)
    class(lagged_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_fqv(f%ep%Np,f%ntau,f%window,int(f%smp(w),8),f%g%nq,f%raw(:,:,w),f%b)
    if (f%self) call normalize_msd(f%ep%Np,f%ntau,f%window,int(f%smp(w),8),f%draw(:,:,w),f%bm)
    call shell_means_lags(f%g%nq,f%g%shell,f%g%nsh,f%g%mult,f%ntau,f%b,f%sh)
    call series_add(f%sVec,w,f%b,vec)
    if (f%self) call series_add(f%sMsd,w,f%bm,vec)
    call series_add(f%sSh,w,f%sh,vec)
    call count_add(f%cnt,vec)
  end subroutine lagged_block

  ! (the shell means are those of the averaged vectors)
  subroutine lagged_average(f,info,vec)
    class(lagged_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%sVec,vec,nall)
       if (f%self) call series_average(f%sMsd,vec,nall)
       call shell_means_lags(f%g%nq,f%g%shell,f%g%nsh,f%g%mult,f%ntau,f%sVec%mean,f%sh)
       call series_add_mean(f%sSh,f%sh)
    end if
  end subroutine lagged_average

  subroutine lagged_write_files(f,suffix,w,n)
    class(lagged_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_fqvec(trim(f%fvec)//'_vpi'//trim(suffix)//'.out',f%ep,f%ntau,f%run%dt,f%g%nq,f%g%n,n,f%sVec%sum(:,w),f%sVec%sq(:,w))
    call write_fqshell(trim(f%fsh)//'_vpi'//trim(suffix)//'.out',f%ntau,f%run%dt,f%g%nsh,f%g%q,f%g%mult,n,f%sSh%sum(:,w),f%sSh%sq(:,w))
    if (f%self) call write_msd('msd_vpi'//trim(suffix)//'.out',f%ep%dim,f%ntau,f%run%dt,n,f%sMsd%sum(:,w),f%sMsd%sq(:,w))
  end subroutine lagged_write_files

  !---------------------------------------------------------------------
  ! tau_profile: the imaginary-time profiles of every slice b = 0..2Nb of a periodic or trapped system -- tau_vpi.out.
  ! Periodic runs also write press_vpi*.out, the virial pressure per block with W averaged over the slices
  ! Nb-tau_window..Nb+tau_window: per walker, and the walker average where there are several.

  subroutine tau_check(f,keys,dim,Nb,trap)
    class(tau_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    call check_window('tau_profile','tau',keys%tau_window,Nb)
    if (.not. tau_bind()) call no_backend('tau_profile','pigs_tau_init / _accumulate / _read','the imaginary-time profiles run')
  end subroutine tau_check

  subroutine tau_banner(f,keys,trap)
    class(tau_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    if (trap) then
       print '(a)', '  > V(tau) profiles     : on (slices 0..2Nb: tau_vpi.out)'
    else
       print '(a,i0,a,i0,a)', '  > V(tau) profiles     : on (slices 0..2Nb: tau_vpi.out; pressure over slices Nb-',keys%tau_window,'..Nb+',keys%tau_window, &
            & ': press_vpi.out)'
    end if
  end subroutine tau_banner

  subroutine tau_setup(f,keys,run,ctx,ep,NW,nvec)
    class(tau_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    integer :: w
    call family_begin(f,run,ep,NW)
    f%window = keys%tau_window
    allocate (f%raw(4,2*run%Nb+1,NW),f%b(4,2*run%Nb+1))
    call series_create(f%s,4*(2*run%Nb+1),NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(tau_init(ctx),'pigs_tau_init')
    f%accumulate => tau_accumulate; f%entry = 'pigs_tau_accumulate'
    if (.not. ep%trap) then
       allocate (f%up(0:NW))
       do w=1,NW
          open (newunit=f%up(w),file='press_vpi'//trim(run%suffix(w))//'.out')
          call press_header(f%up(w),f%window)
       end do
       if (run%averages) then
          open (newunit=f%up(0),file='press_vpi.out')
          call press_header(f%up(0),f%window)
       end if
    end if
  end subroutine tau_setup

  subroutine tau_read_block(f,ctx)
    class(tau_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(tau_read(ctx,f%raw,f%smp,f%reset),'pigs_tau_read')
  end subroutine tau_read_block

  subroutine tau_block(f,w,info,vec)
    class(tau_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    real(8) :: wwin
    call normalize_tau(f%ep%dim,f%ep%Np,f%run%Nb,f%run%dt,int(f%smp(w),8),f%raw(:,:,w),f%b)
    call series_add(f%s,w,f%b,vec)
    call count_add(f%cnt,vec)
    if (.not. f%ep%trap) then
       ! W/Np over the window, the block's Kin/N of e_vpi.out, P = density/dim (2 Kin/N - W/N)
       wwin = virial_window(f%run%Nb,f%window,f%b)
       write (f%up(w),'(20g20.10e3)') real(info%iblock),wwin,info%kin,f%run%density/real(f%ep%dim,8)*(2.d0*(info%kin)-wwin)
    end if
  end subroutine tau_block

  subroutine tau_average(f,info,vec)
    class(tau_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    real(8) :: wwin
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%s,vec,nall)
       if (.not. f%ep%trap .and. info%ndall>0) then
          wwin = virial_window(f%run%Nb,f%window,f%s%mean)
          write (f%up(0),'(20g20.10e3)') real(info%iblock),wwin,info%kin,f%run%density/real(f%ep%dim,8)*(2.d0*(info%kin)-wwin)
       end if
    end if
  end subroutine tau_average

  subroutine tau_write_files(f,suffix,w,n)
    class(tau_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_tau('tau_vpi'//trim(suffix)//'.out',f%run%Nb,f%run%dt,n,f%s%sum(:,w),f%s%sq(:,w))
    if (.not. f%ep%trap) close (f%up(w))
  end subroutine tau_write_files

  !---------------------------------------------------------------------
  ! bond_order: the bond-orientational order of a periodic system in 2D or 3D over the slices Nb-bo_window..Nb+bo_window,
  ! bonds closer than bo_rnb -- bo_vpi.out (Q4, Q6, the means of q4(i), q6(i), the coordination), boh_vpi.out (the
  ! distributions of q4(i), q6(i) on bo_nhist bins) and g6_vpi.out (G6(r) on bo_nr bins up to rcut, gr_vpi.out's format)

  subroutine bop_check(f,keys,dim,Nb,trap)
    class(bop_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('bond_order','its bonds are minimum images in the box')
    if (dim<2) then
       write (0,'(a,i0)') ' pigs_vpi: bond_order = T needs dim = 2 or 3: there is no bond orientation in dim = ',dim
       stop 2
    end if
    if (.not. (keys%bo_rnb>0.d0) .or. keys%bo_rnb>keys%half_side) then
       write (0,'(a,g0,a,g0)') ' pigs_vpi: bond_order = T: bo_rnb = ',keys%bo_rnb, &
            & ' (required) must be positive and at most half the shortest side of the box = ',keys%half_side
       stop 2
    end if
    if (keys%bo_nhist<1 .or. keys%bo_nhist>4096) then
       write (0,'(a,i0,a)') ' pigs_vpi: bond_order = T: bo_nhist = ',keys%bo_nhist,' must lie in 1 .. 4096'
       stop 2
    end if
    if (keys%bo_nr>8192) then
       write (0,'(a,i0,a)') ' pigs_vpi: bond_order = T: bo_nr = ',keys%bo_nr,' must lie in 0 .. 8192 (left out: the g(r) grid)'
       stop 2
    end if
    call check_window('bond_order','bo',keys%bo_window,Nb)
    if (.not. bop_bind()) call no_backend('bond_order','pigs_bop_init / _accumulate / _read','the bond-orientational order runs')
  end subroutine bop_check

  subroutine bop_banner(f,keys,trap)
    class(bop_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,g0.6,a,i0,a,i0,a)', '  > Bond order Q4, Q6   : on (bonds below ',keys%bo_rnb,', slices Nb-',keys%bo_window,'..Nb+',keys%bo_window, &
         & ': bo_vpi.out, boh_vpi.out, g6_vpi.out)'
  end subroutine bop_banner

  subroutine bop_setup(f,keys,run,ctx,ep,NW,nvec)
    class(bop_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    call family_begin(f,run,ep,NW)
    f%nh = keys%bo_nhist; f%window = keys%bo_window; f%rnb = keys%bo_rnb
    f%epr = ep
    if (keys%bo_nr>=0) then
       f%epr%Nbin = keys%bo_nr
       if (keys%bo_nr>0) f%epr%rbin = run%rcut/real(keys%bo_nr,8)
    end if
    f%nr = f%epr%Nbin
    allocate (f%rawS(8,NW),f%H(f%nh,2,NW),f%rawG(max(f%nr,1),NW),f%GN(max(f%nr,1),NW),f%b(5),f%bh(f%nh,2),f%bg(f%nr))
    call series_create(f%sB,5,NW,nvec)
    call series_create(f%sH,2*f%nh,NW,nvec)
    call series_create(f%sG,f%nr,NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(bop_init(ctx,real(f%rnb,c_double),int(f%window,c_int32_t),int(f%nh,c_int32_t),int(f%nr,c_int32_t), &
         & real(f%epr%rbin,c_double)),'pigs_bop_init')
    f%accumulate => bop_accumulate; f%entry = 'pigs_bop_accumulate'
  end subroutine bop_setup

  subroutine bop_read_block(f,ctx)
    class(bop_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(bop_read(ctx,f%rawS,f%H,f%rawG,f%GN,f%smp,f%reset),'pigs_bop_read')
  end subroutine bop_read_block

  subroutine bop_block(f,w,info,vec)
    class(bop_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_bop(f%ep%Np,f%window,int(f%smp(w),8),f%nh,f%nr,f%rawS(:,w),f%H(:,:,w),f%rawG(1:f%nr,w),f%GN(1:f%nr,w), &
         & f%b,f%bh,f%bg)
    call series_add(f%sB,w,f%b,vec)
    call series_add(f%sH,w,f%bh,vec)
    call series_add(f%sG,w,f%bg,vec)
    call count_add(f%cnt,vec)
  end subroutine bop_block

  subroutine bop_average(f,info,vec)
    class(bop_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%sB,vec,nall)
       call series_average(f%sH,vec,nall)
       call series_average(f%sG,vec,nall)
    end if
  end subroutine bop_average

  subroutine bop_write_files(f,suffix,w,n)
    class(bop_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_bo('bo_vpi'//trim(suffix)//'.out',n,f%sB%sum(:,w),f%sB%sq(:,w))
    call write_boh('boh_vpi'//trim(suffix)//'.out',f%nh,n,f%sH%sum(:,w),f%sH%sq(:,w))
    call write_radial('g6_vpi'//trim(suffix)//'.out',f%epr,n,f%sG%sum(:,w),f%sG%sq(:,w))
  end subroutine bop_write_files

  !---------------------------------------------------------------------
  ! van_hove: the van Hove functions of a periodic system for the lags 0..vh_ntau between the slices
  ! Nb-vh_window..Nb+vh_window -- gd_vpi.out (the distinct part on the run's own Nbin/rbin grid) and gs_vpi.out (the self
  ! part on vh_nself bins over [0, vh_rself)), one line per (lag, bin): tau_l, r, G and its error

  subroutine vh_check(f,keys,dim,Nb,trap)
    class(vh_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('van_hove','its displacements are minimum images in the box')
    if (keys%vh_nself<1) then
       write (0,'(a,i0,a)') ' pigs_vpi: van_hove = T: vh_nself = ',keys%vh_nself,' must be at least 1'
       stop 2
    end if
    if (.not. (keys%vh_rself<=huge(1.d0))) then
       write (0,'(a,g0,a)') ' pigs_vpi: van_hove = T: vh_rself = ',keys%vh_rself,' must be finite (left out or <= 0: rcut)'
       stop 2
    end if
    call check_lags('van_hove','vh',keys%vh_ntau,keys%vh_window,Nb)
    if (.not. vh_bind()) call no_backend('van_hove','pigs_vh_init / _accumulate / _read','the van Hove functions run')
  end subroutine vh_check

  subroutine vh_banner(f,keys,trap)
    class(vh_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,i0,a,i0,a,i0,a)', '  > Van Hove G_s, G_d   : on (lags 0..',keys%vh_ntau,', slices Nb-',keys%vh_window,'..Nb+',keys%vh_window, &
         & ': gd_vpi.out, gs_vpi.out)'
  end subroutine vh_banner

  subroutine vh_setup(f,keys,run,ctx,ep,NW,nvec)
    class(vh_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    call family_begin(f,run,ep,NW)
    f%ntau = keys%vh_ntau; f%window = keys%vh_window; f%ns = keys%vh_nself
    f%eps = ep
    f%eps%Nbin = f%ns
    f%eps%rbin = merge(keys%vh_rself,run%rcut,keys%vh_rself>0.d0)/real(f%ns,8)
    call pigs_check(vh_init(ctx,int(f%ntau,c_int32_t),int(f%window,c_int32_t),int(ep%Nbin,c_int32_t),real(ep%rbin,c_double), &
         & int(f%ns,c_int32_t),real(f%eps%rbin,c_double)),'pigs_vh_init')
    f%accumulate => vh_accumulate; f%entry = 'pigs_vh_accumulate'
    allocate (f%cself(f%ns,0:f%ntau,NW),f%cdist(ep%Nbin,0:f%ntau,NW),f%bs(f%ns,0:f%ntau),f%bd(ep%Nbin,0:f%ntau))
    call series_create(f%sS,f%ns*(f%ntau+1),NW,nvec)
    call series_create(f%sD,ep%Nbin*(f%ntau+1),NW,nvec)
    call count_create(f%cnt,nvec)
  end subroutine vh_setup

  subroutine vh_read_block(f,ctx)
    class(vh_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(vh_read(ctx,f%cself,f%cdist,f%smp,f%reset),'pigs_vh_read')
  end subroutine vh_read_block

  subroutine vh_block(f,w,info,vec)
    class(vh_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_vh(f%ep,f%eps,f%run%density,f%window,int(f%smp(w),8),f%ntau,f%cself(:,:,w),f%cdist(:,:,w),f%bs,f%bd)
    call series_add(f%sS,w,reshape(f%bs,[size(f%bs)]),vec)
    call series_add(f%sD,w,reshape(f%bd,[size(f%bd)]),vec)
    call count_add(f%cnt,vec)
  end subroutine vh_block

  subroutine vh_average(f,info,vec)
    class(vh_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%sS,vec,nall)
       call series_average(f%sD,vec,nall)
    end if
  end subroutine vh_average

  subroutine vh_write_files(f,suffix,w,n)
    class(vh_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_vh('gd_vpi'//trim(suffix)//'.out',f%ep,f%run%dt,f%ntau,n,f%sD%sum(:,w),f%sD%sq(:,w))
    call write_vh('gs_vpi'//trim(suffix)//'.out',f%eps,f%run%dt,f%ntau,n,f%sS%sum(:,w),f%sS%sq(:,w))
  end subroutine vh_write_files

  !---------------------------------------------------------------------
  ! triplet: the triplet distribution of a periodic system in 2D or 3D over the slices Nb-g3_window..Nb+g3_window, legs
  ! closer than g3_rmax on g3_nr radial bins, the angle between two legs on g3_na bins of cos(theta) -- g3_vpi.out (one line
  ! per (lo, hi, q): r_lo, r_hi, cos(theta), g3 and its error) and g3ang_vpi.out (P(cos theta) of the legs below g3_rmax)

  subroutine g3_check(f,keys,dim,Nb,trap)
    class(g3_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('triplet','its legs are minimum images in the box')
    if (dim<2) then
       write (0,'(a,i0)') ' pigs_vpi: triplet = T needs dim = 2 or 3: there is no angle between two legs in dim = ',dim
       stop 2
    end if
    if (keys%g3_nr<1 .or. keys%g3_nr>1024) then
       write (0,'(a,i0,a)') ' pigs_vpi: triplet = T: g3_nr = ',keys%g3_nr,' must lie in 1 .. 1024'
       stop 2
    end if
    if (keys%g3_na<1 .or. keys%g3_na>1024) then
       write (0,'(a,i0,a)') ' pigs_vpi: triplet = T: g3_na = ',keys%g3_na,' must lie in 1 .. 1024'
       stop 2
    end if
    if (.not. (keys%g3_rmax>0.d0)) keys%g3_rmax = keys%half_side        ! left out: the run's rcut
    if (.not. (keys%g3_rmax<=keys%half_side)) then
       write (0,'(a,g0,a,g0)') ' pigs_vpi: triplet = T: g3_rmax = ',keys%g3_rmax, &
            & ' must be at most half the shortest side of the box = ',keys%half_side
       stop 2
    end if
    if (keys%g3_window<0) keys%g3_window = 0
    call check_window('triplet','g3',keys%g3_window,Nb)
    if (.not. g3_bind()) call no_backend('triplet','pigs_g3_init / _accumulate / _read','the triplet distribution runs')
  end subroutine g3_check

  subroutine g3_banner(f,keys,trap)
    class(g3_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,g0.6,a,i0,a,i0,a)', '  > Triplet g3          : on (legs below ',keys%g3_rmax,', slices Nb-',keys%g3_window,'..Nb+',keys%g3_window, &
         & ': g3_vpi.out, g3ang_vpi.out)'
  end subroutine g3_banner

  subroutine g3_setup(f,keys,run,ctx,ep,NW,nvec)
    class(g3_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    call family_begin(f,run,ep,NW)
    f%na = keys%g3_na; f%window = keys%g3_window
    f%epr = ep
    f%epr%Nbin = keys%g3_nr
    f%epr%rbin = merge(keys%g3_rmax,run%rcut,keys%g3_rmax>0.d0)/real(keys%g3_nr,8)
    f%npk = keys%g3_nr*(keys%g3_nr+1)/2
    call pigs_check(g3_init(ctx,int(f%epr%Nbin,c_int32_t),real(f%epr%rbin,c_double),int(f%na,c_int32_t),int(f%window,c_int32_t)), &
         & 'pigs_g3_init')
    f%accumulate => g3_accumulate; f%entry = 'pigs_g3_accumulate'
    allocate (f%ctrip(f%na,f%npk,NW),f%cpair(f%epr%Nbin,NW),f%b2(f%epr%Nbin),f%b3(f%na,f%npk),f%ba(f%na))
    call series_create(f%s3,f%na*f%npk,NW,nvec)
    call series_create(f%sA,f%na,NW,nvec)
    call count_create(f%cnt,nvec)
  end subroutine g3_setup

  subroutine g3_read_block(f,ctx)
    class(g3_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(g3_read(ctx,f%ctrip,f%cpair,f%smp,f%reset),'pigs_g3_read')
  end subroutine g3_read_block

  subroutine g3_block(f,w,info,vec)
    class(g3_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_g3(f%epr,f%run%density,f%window,int(f%smp(w),8),f%na,f%ctrip(:,:,w),f%cpair(:,w),f%b2,f%b3,f%ba)
    call series_add(f%s3,w,reshape(f%b3,[size(f%b3)]),vec)
    call series_add(f%sA,w,f%ba,vec)
    call count_add(f%cnt,vec)
  end subroutine g3_block

  subroutine g3_average(f,info,vec)
    class(g3_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%s3,vec,nall)
       call series_average(f%sA,vec,nall)
    end if
  end subroutine g3_average

  subroutine g3_write_files(f,suffix,w,n)
    class(g3_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_g3('g3_vpi'//trim(suffix)//'.out',f%epr,f%na,n,f%s3%sum(:,w),f%s3%sq(:,w))
    call write_g3ang('g3ang_vpi'//trim(suffix)//'.out',f%na,n,f%sA%sum(:,w),f%sA%sq(:,w))
  end subroutine g3_write_files

  !---------------------------------------------------------------------
  ! three_body: the Axilrod-Teller-Muto (triple-dipole) energy of a periodic system in 2D or 3D, evaluated on the sampled
  ! configurations over the slices Nb-atm_window..Nb+atm_window, every side of a triplet within atm_rc -- v3_vpi*.out (one
  ! line per block: V3/Np over the window and its pressure P3; per walker, and the walker average where there are several)
  ! and v3tau_vpi.out (one line per window slice: a, tau, V3/Np and its error, the mean number of triplets)

  subroutine atm_check(f,keys,dim,Nb,trap)
    class(atm_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('three_body','the sides of its triplets are minimum images in the box')
    if (dim<2) then
       write (0,'(a,i0)') ' pigs_vpi: three_body = T needs dim = 2 or 3: there is no triangle in dim = ',dim
       stop 2
    end if
    if (.not. (keys%atm_rc>0.d0)) keys%atm_rc = keys%half_side          ! left out: half the shortest side
    if (.not. (keys%atm_rc<=keys%half_side)) then
       write (0,'(a,g0,a,g0)') ' pigs_vpi: three_body = T: atm_rc = ',keys%atm_rc, &
            & ' must be at most half the shortest side of the box = ',keys%half_side
       stop 2
    end if
    if (keys%atm_window<0) keys%atm_window = 0
    call check_window('three_body','atm',keys%atm_window,Nb)
    if (.not. atm_bind()) call no_backend('three_body','pigs_atm_init / _accumulate / _read','the three-body energy runs')
  end subroutine atm_check

  subroutine atm_banner(f,keys,trap)
    class(atm_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    if (keys%atm_nu_given) then
       print '(a,g0.6,a,g0.6,a,i0,a,i0,a)', '  > Three-body V3       : on (nu = ',keys%atm_nu,', sides below ',keys%atm_rc,', slices Nb-', &
            & keys%atm_window,'..Nb+',keys%atm_window,': v3_vpi.out, v3tau_vpi.out)'
    else
       print '(a,g0.6,a,i0,a,i0,a)', '  > Three-body V3       : on (atm_nu left out: nu = 1, the files hold the bare geometric sum; sides below ', &
            & keys%atm_rc,', slices Nb-',keys%atm_window,'..Nb+',keys%atm_window,': v3_vpi.out, v3tau_vpi.out)'
    end if
  end subroutine atm_banner

  subroutine atm_setup(f,keys,run,ctx,ep,NW,nvec)
    class(atm_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    integer :: w,ns
    call family_begin(f,run,ep,NW)
    f%window = max(keys%atm_window,0)
    f%nu = keys%atm_nu
    f%rc = merge(keys%atm_rc,keys%half_side,keys%atm_rc>0.d0)
    ns = 2*f%window+1
    allocate (f%raw(ns,NW),f%ntrip(ns,NW),f%b(2,ns))
    call series_create(f%s,2*ns,NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(atm_init(ctx,real(f%rc,c_double),int(f%window,c_int32_t)),'pigs_atm_init')
    f%accumulate => atm_accumulate; f%entry = 'pigs_atm_accumulate'
    allocate (f%up(0:NW))
    do w=1,NW
       open (newunit=f%up(w),file='v3_vpi'//trim(run%suffix(w))//'.out')
       call v3_header(f%up(w),f%window)
    end do
    if (run%averages) then
       open (newunit=f%up(0),file='v3_vpi.out')
       call v3_header(f%up(0),f%window)
    end if
  end subroutine atm_setup

  subroutine atm_read_block(f,ctx)
    class(atm_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(atm_read(ctx,f%raw,f%ntrip,f%smp,f%reset),'pigs_atm_read')
  end subroutine atm_read_block

  subroutine atm_block(f,w,info,vec)
    class(atm_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_atm(f%ep%Np,f%window,f%nu,int(f%smp(w),8),f%raw(:,w),int(f%ntrip(:,w),8),f%b)
    call series_add(f%s,w,reshape(f%b,[size(f%b)]),vec)
    call count_add(f%cnt,vec)
    call write_v3_block(f%up(w),info%iblock,f%ep%dim,f%run%density,atm_window_mean(f%window,f%b))
  end subroutine atm_block

  subroutine atm_average(f,info,vec)
    class(atm_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%s,vec,nall)
       if (info%ndall>0) call write_v3_block(f%up(0),info%iblock,f%ep%dim,f%run%density,atm_window_mean(f%window,f%s%mean))
    end if
  end subroutine atm_average

  subroutine atm_write_files(f,suffix,w,n)
    class(atm_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_v3tau('v3tau_vpi'//trim(suffix)//'.out',f%run%Nb,f%window,f%run%dt,n,f%s%sum(:,w),f%s%sq(:,w))
    close (f%up(w))
  end subroutine atm_write_files

  !---------------------------------------------------------------------
  ! momentum: the momentum distribution n(k) of a periodic system with the worm sector on, on the box-commensurate vectors
  ! |n_k| <= nk_nmax, the condensate fraction and the one-body density matrix on nk_nbin bins per axis of the minimum-image
  ! cell -- nkvec_vpi.out (one line per vector, n = 0 first), nk_vpi.out (one line per |k| shell), n0_vpi.out (one line per
  ! block) and nrvec_vpi.out (one line per bin), normalised in the blocks and with the zconf of nr_vpi.out

  subroutine nk_check(f,keys,dim,Nb,trap)
    class(nk_family), intent(inout)  :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    integer :: nbmax
    if (trap) call needs_periodic('momentum','in a trap the one-body density matrix is not translation-invariant')
    if (.not. (keys%cworm>0.d0)) then
       write (0,'(a)') ' pigs_vpi: momentum = T needs the worm sector (CWorm > 0): its samples are the open worldlines'
       stop 2
    end if
    call check_vectors('momentum','nk',keys%nk_nmax,dim)
    nbmax = merge(128,merge(1024,4096,dim==2),dim==3)
    if (keys%nk_nbin<1 .or. keys%nk_nbin>nbmax) then
       write (0,'(a,i0,a,i0,a,i0,a)') ' pigs_vpi: momentum = T: nk_nbin = ',keys%nk_nbin,' must lie in 1 .. ',nbmax,' (dim = ',dim,')'
       stop 2
    end if
    if (.not. nk_bind()) call no_backend('momentum','pigs_nk_init / _count / _vectors / _accumulate / _add / _read', &
         & 'the momentum distribution runs')
  end subroutine nk_check

  subroutine nk_banner(f,keys,trap)
    class(nk_family), intent(in)  :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,i0,a,i0,a)', '  > Momentum n(k), n0   : on (|n_k| <= ',keys%nk_nmax,', ',keys%nk_nbin, &
         & ' bins per axis: nkvec_vpi.out, nk_vpi.out, n0_vpi.out, nrvec_vpi.out)'
  end subroutine nk_banner

  subroutine nk_setup(f,keys,run,ctx,ep,NW,nvec)
    class(nk_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    integer :: w
    call family_begin(f,run,ep,NW)
    f%nbin = keys%nk_nbin
    f%nobdm = keys%nobdm
    f%nv = f%nbin**ep%dim
    call pigs_check(nk_init(ctx,int(keys%nk_nmax,c_int32_t),int(f%nbin,c_int32_t)),'pigs_nk_init')
    call qgrid_fill(f%g,ctx,ep,nk_count,nk_vectors,'pigs_nk')
    allocate (f%raw(f%g%nq,NW),f%h(f%nv,NW),f%nopen(NW),f%nin(NW),f%b(f%g%nq+1),f%sh(f%g%nsh),f%br(f%nv),f%nbl(NW),f%un(0:NW))
    f%nbl = 0
    call series_create(f%sVec,f%g%nq+1,NW,nvec)
    call series_create(f%sSh,f%g%nsh,NW)
    call series_create(f%sR,f%nv,NW,nvec)
    call count_create(f%cnt,nvec)
    do w=1,NW
       open (newunit=f%un(w),file='n0_vpi'//trim(run%suffix(w))//'.out')
       call n0_header(f%un(w))
    end do
    if (run%averages) then
       open (newunit=f%un(0),file='n0_vpi.out')
       call n0_header(f%un(0))
    end if
  end subroutine nk_setup

  ! (the diagonal walkers of a step bring no sample: see set_nk_step, set_nk_add)
  subroutine nk_queue(f,ctx,nd,wl)
    class(nk_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    integer, intent(in)     :: nd
    integer(c_int32_t), intent(in) :: wl(:)
  end subroutine nk_queue

  ! (set_nk_read)
  subroutine nk_read_nothing(f,ctx)
    class(nk_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
  end subroutine nk_read_nothing

  ! (set_nk_block)
  subroutine nk_block_nothing(f,w,info,vec)
    class(nk_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
  end subroutine nk_block_nothing

  ! (the shell means are those of the averaged vectors)
  subroutine nk_average(f,info,vec)
    class(nk_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%sVec,vec,nall)
       call series_average(f%sR,vec,nall)
       call sqv_shell_means(f%g%nq,f%g%shell,f%g%nsh,f%g%mult,f%sVec%mean(2:),f%sh)
       call series_add_mean(f%sSh,f%sh)
       call write_n0_block(f%un(0),info%iblock,f%ep%Np,f%sVec%mean(1))
    end if
  end subroutine nk_average

  subroutine nk_write_files(f,suffix,w,n)
    class(nk_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    integer :: nb
    ! a walker's n are the blocks it counted as diagonal: its files here average over those it normalised (set_nk_block)
    nb = n
    if (w>0) nb = f%nbl(w)
    call write_nkvec('nkvec_vpi'//trim(suffix)//'.out',f%ep,f%g%nq,f%g%n,nb,f%sVec%sum(:,w),f%sVec%sq(:,w))
    call write_sqshell('nk_vpi'//trim(suffix)//'.out',f%g%nsh,f%g%q,f%g%mult,nb,f%sSh%sum(:,w),f%sSh%sq(:,w))
    call write_grvec('nrvec_vpi'//trim(suffix)//'.out',f%ep,f%nbin,f%nv,nb,f%sR%sum(:,w),f%sR%sq(:,w))
    close (f%un(w))
  end subroutine nk_write_files

  !---------------------------------------------------------------------
  ! lattice: a crystal seen from the lattice of config_ini.in, over the slices Nb-lat_window..Nb+lat_window of a periodic
  ! system in 2D or 3D -- lind_vpi*.out (one line per block: <u^2>, the Lindemann ratio, alpha_2, the vacant and the
  ! multiply occupied fraction of the sites, the hops per particle and link and across the window; per walker, and the
  ! walker average where there are several), lindtau_vpi.out (one line per window slice: tau, <u^2>, <u_k^2>, gamma) and
  ! usite_vpi.out (one line per bin: r, rho_site(r), P(u_k = -r) and P(u_k = +r) per axis)

  subroutine lat_check(f,keys,dim,Nb,trap)
    class(lat_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    logical :: there
    integer :: u,s,k,ios
    if (trap) call needs_periodic('lattice','a particle reaches its site by a minimum image in the box')
    if (dim<2) then
       write (0,'(a,i0)') ' pigs_vpi: lattice = T needs dim = 2 or 3, not dim = ',dim
       stop 2
    end if
    inquire (file='config_ini.in',exist=there)
    if (.not. there) then
       write (0,'(a)') ' pigs_vpi: lattice = T needs the lattice sites: there is no config_ini.in in the run directory'
       stop 2
    end if
    open (newunit=u,file='config_ini.in',status='old')
    read (u,*,iostat=ios) keys%lat_nsite
    if (ios==0) read (u,*,iostat=ios)
    if (ios==0) read (u,*,iostat=ios)
    if (ios/=0 .or. keys%lat_nsite<1) then
       write (0,'(a)') ' pigs_vpi: lattice = T: config_ini.in does not start with a number of sites, the box and the density'
       stop 2
    end if
    if (allocated(keys%lat_sites)) deallocate (keys%lat_sites)
    allocate (keys%lat_sites(dim,keys%lat_nsite))
    do s=1,keys%lat_nsite
       read (u,*,iostat=ios) (keys%lat_sites(k,s),k=1,dim)
       if (ios/=0) then
          write (0,'(a,i0,a,i0)') ' pigs_vpi: lattice = T: config_ini.in ends before site ',s,' of ',keys%lat_nsite
          stop 2
       end if
    end do
    close (u)
    keys%lat_ann = lat_nn_distance(dim,keys%lat_nsite,keys%lat_sites,keys%box(1:dim))
    if (keys%lat_nsite<2 .or. .not. (keys%lat_ann>0.d0)) then
       write (0,'(a)') ' pigs_vpi: lattice = T needs two sites or more, no two of them at the same place'
       stop 2
    end if
    if (keys%lat_nbin<=0) keys%lat_nbin = keys%nbin_run
    if (.not. (keys%lat_rmax>0.d0)) keys%lat_rmax = 0.5d0*keys%lat_ann       ! left out: half the nearest-neighbour distance
    if (keys%lat_window<0) keys%lat_window = 0
    call check_window('lattice','lat',keys%lat_window,Nb)
    if (.not. lat_bind()) call no_backend('lattice','pigs_lat_init / _accumulate / _read','the lattice estimators run')
  end subroutine lat_check

  subroutine lat_banner(f,keys,trap)
    class(lat_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,i0,a,g0.6,a,g0.6,a,i0,a,i0,a,l1,a)', '  > Lattice sites        : on (',keys%lat_nsite,' sites of config_ini.in, a_nn = ', &
         & keys%lat_ann,', displacements below ',keys%lat_rmax,', slices Nb-',keys%lat_window,'..Nb+',keys%lat_window, &
         & ', centre of mass removed: ',keys%lat_cm,': lind_vpi.out, lindtau_vpi.out, usite_vpi.out)'
  end subroutine lat_banner

  subroutine lat_setup(f,keys,run,ctx,ep,NW,nvec)
    class(lat_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    integer :: w,ns,dim
    call family_begin(f,run,ep,NW)
    f%window = max(keys%lat_window,0)
    f%nbin = keys%lat_nbin; f%nsite = keys%lat_nsite; f%rmax = keys%lat_rmax; f%ann = keys%lat_ann
    ns = 2*f%window+1; dim = ep%dim
    allocate (f%mom(2+dim,ns,NW),f%nass(ns,NW),f%occ(4,ns,NW),f%hr(f%nbin,NW),f%hx(2*f%nbin,dim,NW))
    allocate (f%nlost(NW),f%hop1(NW),f%hopw(NW),f%bt(2+dim,ns),f%bu(f%nbin*(1+2*dim)))
    call series_create(f%sL,7,NW,nvec)
    call series_create(f%sT,(2+dim)*ns,NW,nvec)
    call series_create(f%sU,f%nbin*(1+2*dim),NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(lat_init(ctx,int(f%nsite,c_int32_t),keys%lat_sites,int(f%nbin,c_int32_t),real(f%rmax,c_double), &
         & int(f%window,c_int32_t),int(merge(1,0,keys%lat_cm),c_int32_t)),'pigs_lat_init')
    f%accumulate => lat_accumulate; f%entry = 'pigs_lat_accumulate'
    allocate (f%up(0:NW))
    do w=1,NW
       open (newunit=f%up(w),file='lind_vpi'//trim(run%suffix(w))//'.out')
       call lind_header(f%up(w),f%window)
    end do
    if (run%averages) then
       open (newunit=f%up(0),file='lind_vpi.out')
       call lind_header(f%up(0),f%window)
    end if
  end subroutine lat_setup

  subroutine lat_read_block(f,ctx)
    class(lat_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(lat_read(ctx,f%mom,f%nass,f%nlost,f%occ,f%hr,f%hx,f%hop1,f%hopw,f%smp,f%reset),'pigs_lat_read')
  end subroutine lat_read_block

  subroutine lat_block(f,w,info,vec)
    class(lat_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_lat(f%ep%dim,f%ep%Np,f%nsite,f%window,f%nbin,f%ann,f%rmax,f%ep%pi,int(f%smp(w),8),f%mom(:,:,w), &
         & int(f%nass(:,w),8),int(f%occ(:,:,w),8),int(f%hr(:,w),8),int(f%hx(:,:,w),8),int(f%hop1(w),8),int(f%hopw(w),8), &
         & f%bl,f%bt,f%bu)
    call series_add(f%sL,w,f%bl,vec)
    call series_add(f%sT,w,reshape(f%bt,[size(f%bt)]),vec)
    call series_add(f%sU,w,f%bu,vec)
    call count_add(f%cnt,vec)
    call write_lind_block(f%up(w),info%iblock,f%bl)
  end subroutine lat_block

  subroutine lat_average(f,info,vec)
    class(lat_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%sL,vec,nall)
       call series_average(f%sT,vec,nall)
       call series_average(f%sU,vec,nall)
       if (info%ndall>0) call write_lind_block(f%up(0),info%iblock,f%sL%mean)
    end if
  end subroutine lat_average

  subroutine lat_write_files(f,suffix,w,n)
    class(lat_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_lindtau('lindtau_vpi'//trim(suffix)//'.out',f%ep%dim,f%window,f%run%dt,n,f%sT%sum(:,w))
    call write_usite('usite_vpi'//trim(suffix)//'.out',f%ep%dim,f%nbin,f%rmax,n,f%sU%sum(:,w))
    close (f%up(w))
  end subroutine lat_write_files

  !---------------------------------------------------------------------
  ! superfluid: the diffusion of the centre of mass along imaginary time over the slices Nb-sf_window..Nb+sf_window of a
  ! periodic system, every link folded once and the folded links added up -- rhos_vpi.out (one line per lag l >= 1: tau,
  ! Dcm and rhos per axis, their mean) and msdu_vpi.out (one line per lag: tau, the unfolded msd per axis and in total,
  ! the cross term per axis), every value with its error over the blocks; per walker, and walker-averaged

  subroutine sf_check(f,keys,dim,Nb,trap)
    class(sf_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('superfluid','a worldline is unfolded through the periodic box')
    call check_lags('superfluid','sf',keys%sf_ntau,keys%sf_window,Nb)
    if (keys%sf_ntau+1>3072) then
       write (0,'(a,i0,a)') ' pigs_vpi: superfluid = T: sf_ntau = ',keys%sf_ntau,' must lie below 3072'
       stop 2
    end if
    if (.not. sf_bind()) call no_backend('superfluid','pigs_sf_init / _accumulate / _read','the centre-of-mass diffusion runs')
  end subroutine sf_check

  subroutine sf_banner(f,keys,trap)
    class(sf_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,i0,a,i0,a,i0,a)', '  > Superfluid fraction  : on (centre-of-mass diffusion, lags 0..',keys%sf_ntau,', slices Nb-', &
         & keys%sf_window,'..Nb+',keys%sf_window,': rhos_vpi.out, msdu_vpi.out)'
  end subroutine sf_banner

  subroutine sf_setup(f,keys,run,ctx,ep,NW,nvec)
    class(sf_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    call family_begin(f,run,ep,NW)
    f%ntau = keys%sf_ntau; f%window = max(keys%sf_window,0)
    allocate (f%c(ep%dim,0:f%ntau,NW),f%d(ep%dim,0:f%ntau,NW),f%nwrap(NW),f%b(sf_columns(ep%dim),0:f%ntau))
    call series_create(f%s,sf_columns(ep%dim)*(f%ntau+1),NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(sf_init(ctx,int(f%ntau,c_int32_t),int(f%window,c_int32_t)),'pigs_sf_init')
    f%accumulate => sf_accumulate; f%entry = 'pigs_sf_accumulate'
  end subroutine sf_setup

  subroutine sf_read_block(f,ctx)
    class(sf_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(sf_read(ctx,f%c,f%d,f%nwrap,f%smp,f%reset),'pigs_sf_read')
  end subroutine sf_read_block

  subroutine sf_block(f,w,info,vec)
    class(sf_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_sf(f%ep%dim,f%ep%Np,f%ntau,f%window,f%run%dt,f%lam,int(f%smp(w),8),f%c(:,:,w),f%d(:,:,w),f%b)
    call series_add(f%s,w,reshape(f%b,[size(f%b)]),vec)
    call count_add(f%cnt,vec)
  end subroutine sf_block

  subroutine sf_average(f,info,vec)
    class(sf_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) call series_average(f%s,vec,nall)
  end subroutine sf_average

  subroutine sf_write_files(f,suffix,w,n)
    class(sf_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_rhos('rhos_vpi'//trim(suffix)//'.out',f%ep%dim,f%ntau,f%run%dt,n,f%s%sum(:,w),f%s%sq(:,w))
    call write_msdu('msdu_vpi'//trim(suffix)//'.out',f%ep%dim,f%ntau,f%run%dt,n,f%s%sum(:,w),f%s%sq(:,w))
  end subroutine sf_write_files

  !---------------------------------------------------------------------
  ! clusters: the connected components of the bond graph r < cl_rc over the slices Nb-cl_window..Nb+cl_window of a periodic
  ! system -- clus_vpi.out (one line per size s that occurred: n(s), the particle fraction s n(s)/Np, P_largest(s) and
  ! <Rg^2>(s), each with its error over the blocks) and clusblk_vpi.out (one line per block: clusters per slice,
  ! <largest cluster>/Np, the mean cluster size, bonds per particle); per walker, and walker-averaged

  subroutine cl_check(f,keys,dim,Nb,trap)
    class(cl_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('clusters','its bonds are minimum images in the box')
    if (keys%cl_rc/=keys%cl_rc .or. abs(keys%cl_rc)>huge(1.d0)) then
       write (0,'(a,g0,a)') ' pigs_vpi: clusters = T: cl_rc = ',keys%cl_rc,' must be finite (left out or <= 0: rcut)'
       stop 2
    end if
    if (.not. (keys%cl_rc>0.d0)) keys%cl_rc = keys%half_side            ! left out: the run's rcut
    if (.not. (keys%cl_rc<=keys%half_side)) then
       write (0,'(a,g0,a,g0)') ' pigs_vpi: clusters = T: cl_rc = ',keys%cl_rc, &
            & ' must be at most half the shortest side of the box = ',keys%half_side
       stop 2
    end if
    if (keys%cl_window<0) keys%cl_window = 0
    call check_window('clusters','cl',keys%cl_window,Nb)
    if (.not. cl_bind()) call no_backend('clusters','pigs_cl_init / _accumulate / _read','the cluster labelling runs')
  end subroutine cl_check

  subroutine cl_banner(f,keys,trap)
    class(cl_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,g0,a,i0,a,i0,a)', '  > Clusters             : on (bonds below cl_rc = ',keys%cl_rc,', slices Nb-', &
         & keys%cl_window,'..Nb+',keys%cl_window,': clus_vpi.out, clusblk_vpi.out)'
  end subroutine cl_banner

  subroutine cl_setup(f,keys,run,ctx,ep,NW,nvec)
    class(cl_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    integer :: w
    call family_begin(f,run,ep,NW)
    f%window = max(keys%cl_window,0); f%rc = keys%cl_rc
    allocate (f%nsize(ep%Np,NW),f%nlarge(ep%Np,NW),f%nbond(NW),f%rg2(ep%Np,NW),f%bs(4,ep%Np))
    call series_create(f%s,4*ep%Np,NW,nvec)
    call series_create(f%sb,4,NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(cl_init(ctx,real(f%rc,c_double),int(f%window,c_int32_t)),'pigs_cl_init')
    f%accumulate => cl_accumulate; f%entry = 'pigs_cl_accumulate'
    allocate (f%up(0:NW))
    do w=1,NW
       open (newunit=f%up(w),file='clusblk_vpi'//trim(run%suffix(w))//'.out')
       call clus_header(f%up(w),f%rc,f%window)
    end do
    if (run%averages) then
       open (newunit=f%up(0),file='clusblk_vpi.out')
       call clus_header(f%up(0),f%rc,f%window)
    end if
  end subroutine cl_setup

  subroutine cl_read_block(f,ctx)
    class(cl_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(cl_read(ctx,f%nsize,f%nlarge,f%nbond,f%smp,f%rg2,f%reset),'pigs_cl_read')
  end subroutine cl_read_block

  subroutine cl_block(f,w,info,vec)
    class(cl_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_cl(f%ep%Np,int(f%smp(w),8),int(f%nsize(:,w),8),int(f%nlarge(:,w),8),int(f%nbond(w),8),f%rg2(:,w),f%bs,f%bb)
    call series_add(f%s,w,reshape(f%bs,[size(f%bs)]),vec)
    call series_add(f%sb,w,f%bb,vec)
    call count_add(f%cnt,vec)
    call write_clus_block(f%up(w),info%iblock,f%bb)
  end subroutine cl_block

  subroutine cl_average(f,info,vec)
    class(cl_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%s,vec,nall)
       call series_average(f%sb,vec,nall)
       if (info%ndall>0) call write_clus_block(f%up(0),info%iblock,f%sb%mean)
    end if
  end subroutine cl_average

  subroutine cl_write_files(f,suffix,w,n)
    class(cl_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_clus('clus_vpi'//trim(suffix)//'.out',f%ep%Np,n,f%s%sum(:,w),f%s%sq(:,w))
    close (f%up(w))
  end subroutine cl_write_files

  !---------------------------------------------------------------------
  ! percolation: which clusters of the bond graph r < pc_rc wrap the periodic box, the finite ones with their unfolded
  ! extent, and the persistence of clusters over the lags 0..pc_ntau, over the slices Nb-pc_window..Nb+pc_window --
  ! perc_vpi.out (one line per block), percsz_vpi.out (one line per finite size that occurred) and clpers_vpi.out (one
  ! line per lag); per walker, and walker-averaged

  subroutine pc_check(f,keys,dim,Nb,trap)
    class(pc_family), intent(inout) :: f
    type(family_keys), intent(inout) :: keys
    integer, intent(in) :: dim,Nb
    logical, intent(in) :: trap
    if (trap) call needs_periodic('percolation','a cluster wraps through the faces of the box')
    if (keys%pc_rc/=keys%pc_rc .or. abs(keys%pc_rc)>huge(1.d0)) then
       write (0,'(a,g0,a)') ' pigs_vpi: percolation = T: pc_rc = ',keys%pc_rc,' must be finite (left out or <= 0: rcut)'
       stop 2
    end if
    if (.not. (keys%pc_rc>0.d0)) keys%pc_rc = keys%half_side            ! left out: the run's rcut
    if (.not. (keys%pc_rc<=keys%half_side)) then
       write (0,'(a,g0,a,g0)') ' pigs_vpi: percolation = T: pc_rc = ',keys%pc_rc, &
            & ' must be at most half the shortest side of the box = ',keys%half_side
       stop 2
    end if
    call check_lags('percolation','pc',keys%pc_ntau,keys%pc_window,Nb)
    if (.not. pc_bind()) call no_backend('percolation','pigs_pc_init / _accumulate / _read','the cluster labelling runs')
  end subroutine pc_check

  subroutine pc_banner(f,keys,trap)
    class(pc_family), intent(in) :: f
    type(family_keys), intent(in) :: keys
    logical, intent(in) :: trap
    print '(a,g0,a,i0,a,i0,a,i0,a)', '  > Percolation          : on (bonds below pc_rc = ',keys%pc_rc,', slices Nb-', &
         & keys%pc_window,'..Nb+',keys%pc_window,', lags 0..',keys%pc_ntau,': perc_vpi.out, percsz_vpi.out, clpers_vpi.out)'
  end subroutine pc_banner

  subroutine pc_setup(f,keys,run,ctx,ep,NW,nvec)
    class(pc_family), intent(inout) :: f
    type(family_keys), intent(in) :: keys
    type(family_run), intent(in)  :: run
    type(c_ptr), intent(in)       :: ctx
    type(est_params), intent(in)  :: ep
    integer, intent(in)    :: NW
    integer, intent(inout) :: nvec
    integer :: w
    call family_begin(f,run,ep,NW)
    f%window = max(keys%pc_window,0); f%ntau = keys%pc_ntau; f%rc = keys%pc_rc
    allocate (f%nwrap(8,NW),f%mwrap(8,NW),f%swrap(8,NW),f%nfin(ep%Np,NW),f%rg2u(ep%Np,NW))
    allocate (f%first(f%ntau+1,NW),f%second(f%ntau+1,NW),f%both(f%ntau+1,NW),f%norig(f%ntau+1,NW))   ! (first index: lag l + 1)
    allocate (f%bs(2,ep%Np),f%bp(3,f%ntau+1))                         ! (second index: lag l + 1)
    call series_create(f%ss,2*ep%Np,NW,nvec)
    call series_create(f%sp,3*(f%ntau+1),NW,nvec)
    call series_create(f%sb,7,NW,nvec)
    call count_create(f%cnt,nvec)
    call pigs_check(pc_init(ctx,real(f%rc,c_double),int(f%window,c_int32_t),int(f%ntau,c_int32_t)),'pigs_pc_init')
    f%accumulate => pc_accumulate; f%entry = 'pigs_pc_accumulate'
    allocate (f%up(0:NW))
    do w=1,NW
       open (newunit=f%up(w),file='perc_vpi'//trim(run%suffix(w))//'.out')
       call perc_header(f%up(w),f%rc,f%window)
    end do
    if (run%averages) then
       open (newunit=f%up(0),file='perc_vpi.out')
       call perc_header(f%up(0),f%rc,f%window)
    end if
  end subroutine pc_setup

  subroutine pc_read_block(f,ctx)
    class(pc_family), intent(inout) :: f
    type(c_ptr), intent(in) :: ctx
    call pigs_check(pc_read(ctx,f%nwrap,f%mwrap,f%swrap,f%nfin,f%smp,f%rg2u,f%first,f%second,f%both,f%norig,f%reset), &
         & 'pigs_pc_read')
  end subroutine pc_read_block

  subroutine pc_block(f,w,info,vec)
    class(pc_family), intent(inout) :: f
    integer, intent(in)           :: w
    type(family_info), intent(in) :: info
    real(8), intent(inout)        :: vec(:)
    call normalize_pc(f%ep%Np,f%ep%dim,f%ntau,int(f%smp(w),8),int(f%nwrap(:,w),8),int(f%mwrap(:,w),8),int(f%swrap(:,w),8), &
         & int(f%nfin(:,w),8),f%rg2u(:,w),int(f%first(:,w),8),int(f%second(:,w),8),int(f%both(:,w),8),int(f%norig(:,w),8), &
         & f%bb,f%bs,f%bp)
    call series_add(f%ss,w,reshape(f%bs,[size(f%bs)]),vec)
    call series_add(f%sp,w,reshape(f%bp,[size(f%bp)]),vec)
    call series_add(f%sb,w,f%bb,vec)
    call count_add(f%cnt,vec)
    call write_perc_block(f%up(w),info%iblock,f%bb)
  end subroutine pc_block

  subroutine pc_average(f,info,vec)
    class(pc_family), intent(inout) :: f
    type(family_info), intent(in) :: info
    real(8), intent(in)           :: vec(:)
    integer :: nall
    nall = count_reduced(f%cnt,vec)
    if (nall>0) then
       call series_average(f%ss,vec,nall)
       call series_average(f%sp,vec,nall)
       call series_average(f%sb,vec,nall)
       if (info%ndall>0) call write_perc_block(f%up(0),info%iblock,f%sb%mean)
    end if
  end subroutine pc_average

  subroutine pc_write_files(f,suffix,w,n)
    class(pc_family), intent(inout) :: f
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,n
    call write_percsz('percsz_vpi'//trim(suffix)//'.out',f%ep%Np,n,f%ss%sum(:,w),f%ss%sq(:,w))
    call write_clpers('clpers_vpi'//trim(suffix)//'.out',f%ntau,f%run%dt,n,f%sp%sum(:,w),f%sp%sq(:,w))
    close (f%up(w))
  end subroutine pc_write_files

end module pigs_families
