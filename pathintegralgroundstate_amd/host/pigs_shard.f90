!-----------------------------------------------------------------------
! pigs_shard -- the state of one walker shard of the front end (pigs_vpi.f90), by what it is for.
!
!     move_counts         accepted and tried moves per walker of a block, from the host's movers or the device's counters
!     energy_sums         block and run sums of the energies per walker, and which blocks a walker counted
!     pending_estimators  the diagonal estimators of a step, queued and collected one step later
!     core_stats          g(r), S(k) and n(r) of the reference: their sums, normalisation, block statistics and files,
!                         in the phases of an estimator family (pigs_families) -- block, average, write_walker,
!                         write_average.  They are no families: the diagonal-estimator call and the OBDM loop feed them,
!                         not a queue / read pair.
!     device_handover     what the device-resident sampler hands over: counters, event log, OBDM histogram, worm state
!     block_totals        what the shards' all-reduce leaves of a block for the report and the averaged energy files
!     shard_state         all of them, with the sampler, the families and the open units
!
! A shard's state is a local of the procedure that the front end calls inside its parallel region: nothing here is saved.
! The procedures that need the run's inputs (namelists) are internal to the program; the ones here need none.
!-----------------------------------------------------------------------
module pigs_shard

  use iso_c_binding
  use pigs_sampler
  use pigs_estimators
  use pigs_block_stats
  use pigs_families

  implicit none
  private
  public :: move_counts,energy_sums,pending_estimators,core_stats,device_handover,block_totals,shard_state
  public :: ACC_CM,ACC_HEAD,ACC_TAIL,ACC_BD,TRY_OPEN,ACC_OPEN,TRY_CLOSE,ACC_CLOSE,ACC_CM_HALF,ACC_HEAD_HALF,ACC_TAIL_HALF
  public :: ACC_BD_HALF,TRY_SWAP,ACC_SWAP,TRY_CM,TRY_STAG,NDEV_COUNTS
  public :: SUM_ACC_CM,SUM_TRY_CM,SUM_ACC_BD,SUM_ACC_HEAD,SUM_ACC_TAIL,SUM_TRY_STAG,SUM_DIAG,SUM_ACC_OPEN,SUM_TRY_OPEN
  public :: SUM_ACC_CLOSE,SUM_TRY_CLOSE,SUM_ACC_SWAP,SUM_TRY_SWAP,NSUMS

  ! the counters of a walker, in the order of pigs_sampler_counters16 (include/pigs_hip.h; 1-based here).  The first
  ! NINT_COUNTS are what the host's movers count in default integers; the device counts the last two as well, the host
  ! keeps them in doubles like the reference (one per particle and step).
  integer, parameter :: ACC_CM = 1, ACC_HEAD = 2, ACC_TAIL = 3, ACC_BD = 4, TRY_OPEN = 5, ACC_OPEN = 6, TRY_CLOSE = 7, &
       & ACC_CLOSE = 8, ACC_CM_HALF = 9, ACC_HEAD_HALF = 10, ACC_TAIL_HALF = 11, ACC_BD_HALF = 12, TRY_SWAP = 13, &
       & ACC_SWAP = 14, TRY_CM = 15, TRY_STAG = 16
  integer, parameter :: NINT_COUNTS = 14, NDEV_COUNTS = 16

  ! the sums over a shard's walkers that the shards reduce once per block (doubles 8..20 of the block vector, in this
  ! order), SUM_DIAG being the diagonal configurations of the block
  integer, parameter :: SUM_ACC_CM = 1, SUM_TRY_CM = 2, SUM_ACC_BD = 3, SUM_ACC_HEAD = 4, SUM_ACC_TAIL = 5, &
       & SUM_TRY_STAG = 6, SUM_DIAG = 7, SUM_ACC_OPEN = 8, SUM_TRY_OPEN = 9, SUM_ACC_CLOSE = 10, SUM_TRY_CLOSE = 11, &
       & SUM_ACC_SWAP = 12, SUM_TRY_SWAP = 13
  integer, parameter :: NSUMS = 13

  type move_counts
     integer, allocatable :: n(:,:)                 ! [NW,NINT_COUNTS] a column per counter: what a mover takes
     real(8), allocatable :: try_cm(:),try_stag(:)  ! [NW]
   contains
     procedure :: create => counts_create
     procedure :: reset => counts_reset
     procedure :: from_device => counts_from_device
     procedure :: block_sums => counts_block_sums
  end type move_counts

  type energy_sums
     ! [3,NW] E, Kin, Pot (mixed estimator) and Et, Kt, Pot (thermodynamic): sums over the steps of a block and of their
     ! squares, then over the blocks of the block means and of their squares
     real(8), allocatable :: BE(:,:),BE2(:,:),BT(:,:),BT2(:,:),AE(:,:),AE2(:,:),AT(:,:),AT2(:,:)
     ! [NW] diagonal configurations of the run, since the last normalised OBDM block and of the block; blocks with a
     ! diagonal configuration, blocks that normalised the OBDM; configurations in the block's g(r) and S(k)
     integer, allocatable :: idiag(:),idiag_aux(:),idiag_block(:),diag_bl(:),obdm_bl(:),ngr(:)
   contains
     procedure :: create => energy_create
     procedure :: reset => energy_reset
  end type energy_sums

  type pending_estimators
     logical :: queued = .false.                    ! a step's estimators wait to be collected
     logical :: structure = .false.                 ! g(r) and S(k) come with them (device-resident sampler, periodic)
     integer :: nd = 0                              ! of so many diagonal walkers,
     integer, allocatable :: list(:)                ! [NW] these (local index)
     real(8), allocatable :: en9(:,:)               ! [9,NW] LocalEnergy of both ends, ThermEnergy per listed walker
     real(8), allocatable :: gr_inc(:,:),sk_inc(:,:,:)   ! [Nbin,NW], [dim,Nk,NW] the step's histograms from the device
  end type pending_estimators

  type core_stats
     logical :: on = .false.                        ! periodic systems only
     type(est_params) :: ep
     real(8) :: density = 0.d0
     integer :: Nobdm = 0
     real(8), allocatable :: gr(:,:),Sk(:,:,:)      ! [Nbin,NW], [dim,Nk,NW] sums of the block
     real(8), allocatable :: nrho(:,:,:)            ! [0:Npw,Nbin,NW] since the walker's last normalised OBDM block
     ! g(r) and S(k) share the count of the walkers with a diagonal block, n(r) has the one of the walkers whose OBDM
     ! block is full
     type(block_series) :: sGr,sSk,sNr
     type(block_count)  :: cGr,cNr
   contains
     procedure :: create => core_create
     procedure :: reset => core_reset
     procedure :: block => core_block
     procedure :: block_nr => core_block_nr
     procedure :: average => core_average
     procedure :: write_walker => core_write_walker
     procedure :: write_average => core_write_average
  end type core_stats

  type device_handover
     integer(c_int64_t), allocatable :: acc(:,:),acc0(:,:)        ! [16,NW] counters since pigs_sampler_init: now, a block ago
     integer(c_int32_t), allocatable :: ev(:,:)                   ! [pigs_sampler_event_ints,NW] a step's event log
     integer(c_int32_t), allocatable :: isopen(:),iworm(:),reset(:)
     real(8), allocatable :: nrho(:,:,:)
  end type device_handover

  type block_totals
     integer :: ndall = 0                           ! walkers of all shards with a diagonal block
     real(8) :: mE(3) = 0.d0, mT(3) = 0.d0          ! their summed block energies per particle
     real(8) :: moves(NSUMS) = 0.d0                 ! move_counts%block_sums of all shards
  end type block_totals

  type shard_state
     integer :: ish = 0, NW = 0, w0 = 0             ! the shard, its walkers; global walker index = w0 + local index
     type(c_ptr) :: ctx = c_null_ptr
     logical :: trace = .false.
     type(sampler_t)  :: s
     type(est_params) :: ep
     type(perm_state), allocatable :: perm(:)
     type(move_counts) :: moves
     type(energy_sums) :: en
     type(pending_estimators) :: pend
     type(core_stats)  :: core
     type(device_handover) :: dev
     ! the accumulator families of the estimator keys (pigs_families): the shard's own set, what it is told of every block
     type(family_set)  :: fams
     type(family_info) :: info
     ! the vector that meets the other shards' once per block (nvec doubles)
     integer :: nvec = 0
     real(8), allocatable :: vec(:)
     type(block_totals) :: tot
     integer, allocatable :: ue(:),ut(:),uh(:)      ! [NW] e_vpi, et_vpi .out and e_vpi.hex of every walker
     integer :: ueav = -1, utav = -1                ! the walker-averaged e_vpi.out, et_vpi.out (shard 1, several walkers)
  end type shard_state

contains

  !---------------------------------------------------------------------
  ! move_counts

  subroutine counts_create(c,NW)
    class(move_counts), intent(inout) :: c
    integer, intent(in) :: NW
    allocate (c%n(NW,NINT_COUNTS),c%try_cm(NW),c%try_stag(NW))
    call c%reset()
  end subroutine counts_create

  subroutine counts_reset(c)
    class(move_counts), intent(inout) :: c
    c%n = 0; c%try_cm = 0.d0; c%try_stag = 0.d0
  end subroutine counts_reset

  ! the block's counts from the device's, which run since pigs_sampler_init: acc now, acc0 at the end of the previous
  ! block (moved on to acc)
  subroutine counts_from_device(c,acc,acc0)
    class(move_counts), intent(inout) :: c
    integer(c_int64_t), intent(in)    :: acc(:,:)
    integer(c_int64_t), intent(inout) :: acc0(:,:)
    integer :: k
    do k=1,NINT_COUNTS
       c%n(:,k) = int(acc(k,:)-acc0(k,:))
    end do
    c%try_cm   = dble(acc(TRY_CM,:)-acc0(TRY_CM,:))
    c%try_stag = dble(acc(TRY_STAG,:)-acc0(TRY_STAG,:))
    acc0 = acc
  end subroutine counts_from_device

  ! the shard's part of doubles 8..20 of the block vector; ndiag: the diagonal configurations of its walkers' block
  function counts_block_sums(c,ndiag) result(v)
    class(move_counts), intent(in) :: c
    integer, intent(in) :: ndiag
    real(8) :: v(NSUMS)
    v(SUM_ACC_CM)    = dble(sum(c%n(:,ACC_CM)));    v(SUM_TRY_CM)    = sum(c%try_cm)
    v(SUM_ACC_BD)    = dble(sum(c%n(:,ACC_BD)));    v(SUM_TRY_STAG)  = sum(c%try_stag)
    v(SUM_ACC_HEAD)  = dble(sum(c%n(:,ACC_HEAD)));  v(SUM_ACC_TAIL)  = dble(sum(c%n(:,ACC_TAIL)))
    v(SUM_DIAG)      = dble(ndiag)
    v(SUM_ACC_OPEN)  = dble(sum(c%n(:,ACC_OPEN)));  v(SUM_TRY_OPEN)  = dble(sum(c%n(:,TRY_OPEN)))
    v(SUM_ACC_CLOSE) = dble(sum(c%n(:,ACC_CLOSE))); v(SUM_TRY_CLOSE) = dble(sum(c%n(:,TRY_CLOSE)))
    v(SUM_ACC_SWAP)  = dble(sum(c%n(:,ACC_SWAP)));  v(SUM_TRY_SWAP)  = dble(sum(c%n(:,TRY_SWAP)))
  end function counts_block_sums

  !---------------------------------------------------------------------
  ! energy_sums

  subroutine energy_create(e,NW)
    class(energy_sums), intent(inout) :: e
    integer, intent(in) :: NW
    allocate (e%BE(3,NW),e%BE2(3,NW),e%BT(3,NW),e%BT2(3,NW),e%AE(3,NW),e%AE2(3,NW),e%AT(3,NW),e%AT2(3,NW))
    allocate (e%idiag(NW),e%idiag_aux(NW),e%idiag_block(NW),e%diag_bl(NW),e%obdm_bl(NW),e%ngr(NW))
    e%AE = 0.d0; e%AE2 = 0.d0; e%AT = 0.d0; e%AT2 = 0.d0
    e%idiag = 0; e%idiag_aux = 0; e%obdm_bl = 0; e%diag_bl = 0
    call e%reset()
  end subroutine energy_create

  ! start of a block
  subroutine energy_reset(e)
    class(energy_sums), intent(inout) :: e
    e%idiag_block = 0; e%ngr = 0
    e%BE = 0.d0; e%BE2 = 0.d0; e%BT = 0.d0; e%BT2 = 0.d0
  end subroutine energy_reset

  !---------------------------------------------------------------------
  ! core_stats

  ! nvec: the layout counter of the block vector, moved past the three series and the two counts
  subroutine core_create(c,ep,density,Nobdm,NW,nvec)
    class(core_stats), intent(inout) :: c
    type(est_params), intent(in)   :: ep
    real(8), intent(in)    :: density
    integer, intent(in)    :: Nobdm,NW
    integer, intent(inout) :: nvec
    c%on = .not. ep%trap; c%ep = ep; c%density = density; c%Nobdm = Nobdm
    call series_create(c%sGr,ep%Nbin,NW,nvec)
    call series_create(c%sSk,ep%dim*ep%Nk,NW,nvec)
    call series_create(c%sNr,(ep%Npw+1)*ep%Nbin,NW,nvec)
    call count_create(c%cGr,nvec)
    call count_create(c%cNr,nvec)
    allocate (c%gr(ep%Nbin,NW),c%Sk(ep%dim,ep%Nk,NW),c%nrho(0:ep%Npw,ep%Nbin,NW))
    c%nrho = 0.d0
    call c%reset()
  end subroutine core_create

  ! start of a block (n(r) goes on until the block that normalises it)
  subroutine core_reset(c)
    class(core_stats), intent(inout) :: c
    c%gr = 0.d0; c%Sk = 0.d0
  end subroutine core_reset

  ! walker w counted the block, with ngr configurations in its g(r) and S(k)
  subroutine core_block(c,w,ngr,vec)
    class(core_stats), intent(inout) :: c
    integer, intent(in)    :: w,ngr
    real(8), intent(inout) :: vec(:)
    if (.not. c%on) return
    call normalize_gr(c%ep,c%density,ngr,c%gr(:,w))
    call normalize_sk(c%ep,ngr,c%Sk(:,:,w))
    call series_add(c%sGr,w,c%gr(:,w),vec)
    call series_add(c%sSk,w,c%Sk(:,:,w),vec)
    call count_add(c%cGr,vec)
  end subroutine core_block

  ! walker w normalises its OBDM histogram in this block, with zconf diagonal configurations, and starts it anew
  subroutine core_block_nr(c,w,zconf,vec)
    class(core_stats), intent(inout) :: c
    integer, intent(in)    :: w
    real(8), intent(in)    :: zconf
    real(8), intent(inout) :: vec(:)
    if (c%on) then
       call normalize_nr(c%ep,c%density,zconf,c%Nobdm,c%nrho(:,:,w))
       call series_add(c%sNr,w,c%nrho(:,:,w),vec)
       call count_add(c%cNr,vec)
    end if
    c%nrho(:,:,w) = 0.d0
  end subroutine core_block_nr

  ! on the shard that writes the walker averages, after the all-reduce
  subroutine core_average(c,vec)
    class(core_stats), intent(inout) :: c
    real(8), intent(in) :: vec(:)
    integer :: nall
    nall = count_reduced(c%cGr,vec)
    if (nall>0) then
       call series_average(c%sGr,vec,nall)
       call series_average(c%sSk,vec,nall)
    end if
    nall = count_reduced(c%cNr,vec)
    if (nall>0) call series_average(c%sNr,vec,nall)
  end subroutine core_average

  ! the files of walker w (local index), which counted diag_bl diagonal and obdm_bl OBDM blocks: written unconditionally,
  ! like the reference (a run without a single diagonal / OBDM block yields NaN columns there too).  w = 0, suffix = '':
  ! the walker-averaged ones
  subroutine core_write_walker(c,suffix,w,diag_bl,obdm_bl)
    class(core_stats), intent(inout) :: c
    character(len=*), intent(in) :: suffix
    integer, intent(in)          :: w,diag_bl,obdm_bl
    if (.not. c%on) return
    call write_radial('gr_vpi'//trim(suffix)//'.out',c%ep,diag_bl,c%sGr%sum(:,w),c%sGr%sq(:,w))
    call write_sk('sk_vpi'//trim(suffix)//'.out',c%ep,diag_bl,c%sSk%sum(:,w),c%sSk%sq(:,w))
    call write_nr('nr_vpi'//trim(suffix)//'.out',c%ep,obdm_bl,c%sNr%sum(:,w),c%sNr%sq(:,w))
  end subroutine core_write_walker

  ! the walker-averaged histograms, from the reduced block vectors
  subroutine core_write_average(c)
    class(core_stats), intent(inout) :: c
    call c%write_walker('',0,c%cGr%nav,c%cNr%nav)
  end subroutine core_write_average

end module pigs_shard
