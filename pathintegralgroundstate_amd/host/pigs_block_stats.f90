!-----------------------------------------------------------------------
! pigs_block_stats -- the block statistics behind every estimator file of the front end (pigs_vpi.f90).
!
! A block_series is one output file's worth of numbers, flattened to length n: per walker the sum of the block values
! and of their squares (the .wNNNN file, or the only file of a one-walker run), as column 0 the same two moments of the
! walker average of every block (the unsuffixed file of a run with several walkers), and the place of the series in the
! vector that the shards all-reduce once per block: there the block values of the walkers that counted the block are summed, so
! that slice / count is the block's walker average on every shard.  A block_count is the count slot that goes with the
! series of one estimator family, and the number of blocks that at least one walker counted.
!
! The layout of the vector is nobody's business but this module's: every create call claims the next doubles from a
! running counter, whose final value is the vector's length.
!
! The arithmetic is fixed to the bit: sums grow one block value at a time in the order of the calls, squares are b*b,
! the walker average is slice / integer count.
!-----------------------------------------------------------------------
module pigs_block_stats

  implicit none
  private
  public :: block_series,block_count,series_create,series_add,series_average,series_add_mean
  public :: count_create,count_add,count_reduced

  type block_series
     integer :: n   = 0
     integer :: off = -1                            ! the slice is vec(off+1:off+n); < 0: the series has none
     real(8), allocatable :: sum(:,:),sq(:,:)       ! [n,0:NW] per walker: sum of the block values, of their squares;
                                                    ! column 0: the same of the blocks' walker averages
     real(8), allocatable :: mean(:)                ! [n] the walker average of the last block (series_average)
  end type block_series

  type block_count
     integer :: slot = 0                            ! vec(slot): how many walkers of all shards counted the block
     integer :: nav  = 0                            ! blocks that at least one walker counted
  end type block_count

contains

  ! A zeroed series of length n for NW walkers.  With the layout counter nvec it claims the next n doubles of the block
  ! vector; without, it has no slice (a series derived from another one's walker average: the |q|-shell means).
  subroutine series_create(s,n,NW,nvec)
    type(block_series), intent(out)  :: s
    integer, intent(in)              :: n,NW
    integer, intent(inout), optional :: nvec
    s%n = n
    allocate (s%sum(n,0:NW),s%sq(n,0:NW),s%mean(n))
    s%sum = 0.d0; s%sq = 0.d0; s%mean = 0.d0
    if (present(nvec)) then
       s%off = nvec
       nvec  = nvec+n
    end if
  end subroutine series_create

  ! walker w (local index) counts the block with the value b
  subroutine series_add(s,w,b,vec)
    type(block_series), intent(inout) :: s
    integer, intent(in)    :: w
    real(8), intent(in)    :: b(s%n)
    real(8), intent(inout) :: vec(:)
    s%sum(:,w) = s%sum(:,w)+b
    s%sq(:,w)  = s%sq(:,w)+b*b
    if (s%off>=0) vec(s%off+1:s%off+s%n) = vec(s%off+1:s%off+s%n)+b
  end subroutine series_add

  ! the block's walker average from the reduced vector, cnt > 0 walkers having counted it: left in s%mean and added to
  ! the averaged moments
  subroutine series_average(s,vec,cnt)
    type(block_series), intent(inout) :: s
    real(8), intent(in) :: vec(:)
    integer, intent(in) :: cnt
    s%mean = vec(s%off+1:s%off+s%n)/cnt
    s%sum(:,0) = s%sum(:,0)+s%mean
    s%sq(:,0)  = s%sq(:,0)+s%mean*s%mean
  end subroutine series_average

  ! the same for a series without a slice: the caller derived the block's walker average a from another series' mean
  subroutine series_add_mean(s,a)
    type(block_series), intent(inout) :: s
    real(8), intent(in) :: a(s%n)
    s%sum(:,0) = s%sum(:,0)+a
    s%sq(:,0)  = s%sq(:,0)+a*a
  end subroutine series_add_mean

  ! claims one double of the block vector for a family's count
  subroutine count_create(c,nvec)
    type(block_count), intent(out) :: c
    integer, intent(inout)         :: nvec
    nvec   = nvec+1
    c%slot = nvec
  end subroutine count_create

  ! one more walker counted the block
  subroutine count_add(c,vec)
    type(block_count), intent(in) :: c
    real(8), intent(inout)        :: vec(:)
    vec(c%slot) = vec(c%slot)+1.d0
  end subroutine count_add

  ! how many walkers of all shards counted the block, from the reduced vector; a block that somebody counted is one more
  ! averaged block
  integer function count_reduced(c,vec) result(cnt)
    type(block_count), intent(inout) :: c
    real(8), intent(in)              :: vec(:)
    cnt = nint(vec(c%slot))
    if (cnt>0) c%nav = c%nav+1
  end function count_reduced

  ! C-callable handle (no state), for tests of the host logic: NW walkers in two shards, the first NW1 and the rest,
  ! put Nblock block values b(n,NW,Nblock) through one series with a slice and through one without, of length m, whose
  ! value is the sum of b over the elements of equal group(1:n) in 1..m -- per walker of the walker's block value, for
  ! the walker average of the averaged one, as the front end does with the |q|-shell means.  counted(NW,Nblock) /= 0
  ! where the walker counts the block.  Each shard fills a vector of its own; the two are added element by element, as
  ! the all-reduce does, and the first shard takes the walker average.  vec0 is the layout counter before the claims,
  ! nvec after them.
  subroutine bs_series_run(n,NW,NW1,Nblock,m,group,b,counted,vec0,wsum,wsq,asum,asq,gsum,gsq,gasum,gasq,nav,nvec) &
       & bind(C,name='bs_series_run')
    use iso_c_binding
    integer(c_int), value       :: n,NW,NW1,Nblock,m,vec0
    integer(c_int), intent(in)  :: group(n),counted(NW,Nblock)
    real(c_double), intent(in)  :: b(n,NW,Nblock)
    real(c_double), intent(out) :: wsum(n,NW),wsq(n,NW),asum(n),asq(n),gsum(m,NW),gsq(m,NW),gasum(m),gasq(m)
    integer(c_int), intent(out) :: nav,nvec
    type(block_series) :: s(2),g(2)
    type(block_count)  :: c(2)
    real(8), allocatable :: vec(:,:)
    real(8) :: gb(m)
    integer :: lo(2),hi(2),nv,ish,w,ib,cnt
    lo = [1,NW1+1]; hi = [NW1,NW]
    do ish=1,2
       nv = vec0
       call series_create(s(ish),n,hi(ish)-lo(ish)+1,nv)
       call series_create(g(ish),m,hi(ish)-lo(ish)+1)
       call count_create(c(ish),nv)
    end do
    nvec = nv
    allocate (vec(nv,2))
    do ib=1,Nblock
       vec = 0.d0
       do ish=1,2
          do w=lo(ish),hi(ish)
             if (counted(w,ib)==0) cycle
             call group_sums(b(:,w,ib),gb)
             call series_add(s(ish),w-lo(ish)+1,b(:,w,ib),vec(:,ish))
             call series_add(g(ish),w-lo(ish)+1,gb,vec(:,ish))
             call count_add(c(ish),vec(:,ish))
          end do
       end do
       vec(:,1) = vec(:,1)+vec(:,2)
       cnt = count_reduced(c(1),vec(:,1))
       if (cnt>0) then
          call series_average(s(1),vec(:,1),cnt)
          call group_sums(s(1)%mean,gb)
          call series_add_mean(g(1),gb)
       end if
    end do
    do ish=1,2
       wsum(:,lo(ish):hi(ish)) = s(ish)%sum(:,1:); wsq(:,lo(ish):hi(ish)) = s(ish)%sq(:,1:)
       gsum(:,lo(ish):hi(ish)) = g(ish)%sum(:,1:); gsq(:,lo(ish):hi(ish)) = g(ish)%sq(:,1:)
    end do
    asum = s(1)%sum(:,0); asq = s(1)%sq(:,0); gasum = g(1)%sum(:,0); gasq = g(1)%sq(:,0)
    nav = c(1)%nav
  contains
    subroutine group_sums(x,y)
      real(8), intent(in)  :: x(n)
      real(8), intent(out) :: y(m)
      integer :: i
      y = 0.d0
      do i=1,n
         y(group(i)) = y(group(i))+x(i)
      end do
    end subroutine group_sums
  end subroutine bs_series_run

end module pigs_block_stats
